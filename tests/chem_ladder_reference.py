"""A model of the ladder of sub-step ceilings that a heating global pass walks (c2r_global_pass_cells /
c2r_global_pass_finish, "Heating global pass in tiers"), in plain Python.  Not a test module; no GPU, no torch.

It knows nothing of chemistry: it takes W, the thermal sub-steps every cell of the pass needs (the oracle's count,
orc.global_pass_work), and says which launches the pass makes and where the next pass starts.  The rules, as the code has them:

  - a cell is deferred under the ceiling B iff W > B (thermal() gives up when its count PASSES the ceiling);
  - the first launch runs every cell under the pass's first ceiling; after each launch that deferred n > 0 cells the ceiling is
    multiplied by 4 and the n cells are redone;
  - that next launch is unbounded, and the last, if n <= resident, or the new ceiling exceeds 1 024, or it is the fifth
    follow-up launch;
  - histogram bucket b holds the cells with W in [2^(b-1), 2^b), bucket 0 those with W = 0;
  - the next pass's first ceiling is the lowest of 16, 64, 256, 1 024 for which the buckets with 2^b <= rung hold at least half
    of all cells (1 024 if none does); with an empty histogram it goes back to 16.

So a cell with W = 16 finishes under the ceiling 16 but counts in bucket 5, above the rung 16.
"""
FIRST_CEILING, CEILING_STEP, LAST_CEILING, TIERS, NBUCKETS = 16, 4, 1024, 6, 24
RUNGS = (16, 64, 256, 1024)
DEFAULT_RESIDENT = 131072


def deferred(W, ceiling):
    """The cells (positions in W) that a launch under `ceiling` defers; none when it is unbounded (None)."""
    if ceiling is None:
        return []
    return [i for i, w in enumerate(W) if w > ceiling]


def bucket(w):
    """The histogram bucket of a cell that needed w sub-steps: 0 for none, else the b with 2^(b-1) <= w < 2^b."""
    return int(w).bit_length()


def histogram(W):
    h = [0] * NBUCKETS
    for w in W:
        h[bucket(w)] += 1
    return h


def next_first(hist):
    total = sum(hist)
    if total == 0:
        return FIRST_CEILING
    acc, b, first = 0, 0, FIRST_CEILING
    for rung in RUNGS:
        while b < len(hist) and (1 << b) <= rung:
            acc += hist[b]
            b += 1
        first = rung
        if 2 * acc >= total:
            break
    return first


def ladder(W, first=FIRST_CEILING, resident=DEFAULT_RESIDENT):
    """One pass over cells that need W[i] sub-steps, from the first ceiling `first`: (launches, next first ceiling).
    launches = [(ceiling or None for unbounded, cells deferred by that launch), ...], the first launch included."""
    W = [int(w) for w in W]
    left = deferred(W, first)
    launches = [(first, len(left))]
    ceiling = first
    for t in range(1, TIERS):
        n = len(left)
        if n <= 0:
            break
        ceiling *= CEILING_STEP
        last = t == TIERS - 1 or n <= resident or ceiling > LAST_CEILING
        cells = [W[i] for i in left]
        left = [left[i] for i in deferred(cells, None if last else ceiling)]
        launches.append((None if last else ceiling, len(left)))
        if last:
            break
    return launches, next_first(histogram(W))


def chain(Ws, resident=DEFAULT_RESIDENT, first=FIRST_CEILING):
    """The passes of one context, each from the first ceiling the pass before left: [(launches, first ceiling of that pass)]."""
    out = []
    for W in Ws:
        launches, nxt = ladder(W, first, resident)
        out.append((launches, first))
        first = nxt
    return out
