"""The inputs of the ladder tests, shared by tests/test_chem_ladder_host.py (CPU: the cases cover what they claim, by the
oracle's own counts) and tests/test_gpu_chem_ladder.py (GPU: the heating global pass against the oracle, bit for bit).
Not a test module; no GPU, no torch.

Directed case: an isolated global pass on a tiny mesh whose state, temperatures and rates are uploaded -- no ray tracing --
and drawn so wide that the thermal sub-steps per cell span every rung of the ladder of ceilings (16, 64, 256, 1 024, none):
densities over four decades, neutral fractions from 1e-6 to 1 - 1e-6, temperatures 10^-0.5 ... 10^5.5 K, photo-ionisation
rates 1e-18 ... 1e-9 per second with 15 % of the cells at 0, heating = rate x density x 10^(-12.5 ... -9.5).  Three passes on
the same rates at dt = 1e5 yr, and three from the same start at 3e6 yr.  COLD = 35 % of the cells are drawn from the part of
the temperature range at or below minitemp = 1 K: they skip the sub-cycle and count 0 sub-steps, in every pass.  Without them
(temperatures log-uniform over the whole range, a twelfth of the cells cold) fewer than half of the cells stay below 16
sub-steps at 3e6 yr -- in none of 300 draws -- so the second pass would start its ladder at 64 and no longer walk every rung.
The last cell of the mesh exchanges its inputs with the cell of the longest chain (DRAWS: found once with the oracle, held to
by the host test), so that the coefficients the pass leaves behind (rc_last) are written by a late launch.  The seeds are
those of 200 tried per mesh under which the host test's conditions hold at both time steps with the shortest chains.

Ray-traced sequence: the 8 x 4 x 4 two-source heating case of tests/test_gpu_parity.py's wave-shape test (same seed, same draws),
continued to eight outer iterations, over which the first ceiling of the ladder moves by itself.

What the cases must cover is asserted by the host test; MAX_CHAIN bounds the longest chain of any cell in any pass.
"""
import numpy as np

YEAR = 3.15576e7
ZRED = 9.0
TEMPER_VAL = 1.0e4
MESHES = {"ragged": (8, 4, 6), "bricks": (8, 4, 8)}       # six planes: rows only; eight: 8 x 4 x 2 bricks in the first launch
DTS = (1.0e5, 3.0e6)                                      # years
NPASS = 3
DARK = 0.15                                               # share of the cells without radiation
COLD = 0.35                                               # share of the cells that enter at or below minitemp
# per mesh: the seed of the draws, and the cell whose inputs are exchanged with those of the last cell of the mesh
DRAWS = {"ragged": dict(seed=0, long_cell=105), "bricks": dict(seed=96, long_cell=139)}
PIECES = (1, 65, 130)                                     # where the pass in pieces is cut: none a multiple of 64
MAX_CHAIN = 60000                                         # sub-steps of one cell in one pass: a launch stays under 0.1 s
RAY_MESH, RAY_ITERS, RAY_DT = (8, 4, 4), 8, 3.0e6


def directed(hp, name, clump=False, draw=None):
    """The directed case on the mesh MESHES[name]: a dict of arrays and scalars."""
    mesh = MESHES[name]
    draw = draw or DRAWS[name]
    seed = draw["seed"]
    nc = mesh[0] * mesh[1] * mesh[2]
    rng = np.random.default_rng([seed, nc])
    dr, vol = hp.test_grid(16, ZRED)
    ndens = hp.test_density(ZRED) * 10.0 ** rng.uniform(-2.0, 2.0, nc)
    x = 10.0 ** rng.uniform(-6.0, 0.0, nc)                 # neutral fraction ...
    flip = rng.random(nc) < 0.5
    x = np.where(flip, 1.0 - x, x)                         # ... or ionised fraction: both ends to 1e-6
    x = np.clip(x, 1.0e-6, 1.0 - 1.0e-6)
    xh = np.concatenate([x, 1.0 - x])
    y = 1.0 - x
    xhe = np.concatenate([1.0 - y, 0.7 * y, 0.3 * y])
    cold = rng.random(nc) < COLD
    temp1 = (10.0 ** np.where(cold, rng.uniform(-0.5, 0.0, nc), rng.uniform(0.0, 5.5, nc))).astype(np.float32)
    phih = 10.0 ** rng.uniform(-18.0, -9.0, nc)
    phih[rng.random(nc) < DARK] = 0.0
    phihe = np.concatenate([0.5 * phih, 0.05 * phih])
    phiheat = phih * ndens * 10.0 ** rng.uniform(-12.5, -9.5, nc)
    case = dict(mesh=tuple(mesh), ncell=nc, dr=dr, vol=vol, zred=ZRED, ndens=ndens, xh=xh, xhe=xhe, temp=np.tile(temp1, 3),
                phih=phih, phihe=phihe, phiheat=phiheat, reccoef=hp.reccoef(TEMPER_VAL), clumping=1.0,
                clumping_grid=(1.0 + 5.0 * np.random.default_rng([seed, nc, 5]).random(nc)).astype(np.float32) if clump else None,
                srcpos=np.array([[1, 1, 1]], dtype=np.int32), flux=np.array([1.0e6]), s_star=1.0e48)
    swap_cells(case, draw["long_cell"], nc - 1)
    return case


def swap_cells(case, a, b):
    """Cells a and b exchange every input (all components of every grid)."""
    nc = case["ncell"]
    for k, ncomp in (("ndens", 1), ("xh", 2), ("xhe", 3), ("temp", 3), ("phih", 1), ("phihe", 2), ("phiheat", 1), ("clumping_grid", 1)):
        if case[k] is not None:
            for n in range(ncomp):
                case[k][[a + n * nc, b + n * nc]] = case[k][[b + n * nc, a + n * nc]]


def raytraced(hp):
    """Case "b" of tests/test_gpu_parity.py's _CHEM_SNIPPET, draw for draw."""
    mesh = RAY_MESH
    nc = mesh[0] * mesh[1] * mesh[2]
    rng = np.random.default_rng(3 + mesh[0] + mesh[2])
    dr, vol = hp.test_grid(16, ZRED)
    ndens = hp.test_density(ZRED) * np.exp(rng.normal(0.0, 0.5, nc))
    x = 10.0 ** rng.uniform(-5, -0.5, nc)
    xh = np.concatenate([1.0 - x, x])
    xhe = np.concatenate([1.0 - x, 0.7 * x, 0.3 * x])
    temp = np.tile((1e4 * np.exp(rng.normal(0, 0.2, nc))).astype(np.float32), 3)
    srcpos = np.array([[1, mesh[1], mesh[2] // 2], [mesh[0] // 2, 3, mesh[2]]], dtype=np.int32)
    return dict(mesh=mesh, ncell=nc, dr=dr, vol=vol, zred=ZRED, ndens=ndens, xh=xh, xhe=xhe, temp=temp, reccoef=hp.reccoef(TEMPER_VAL),
                clumping=1.0, clumping_grid=None, srcpos=srcpos, flux=np.array([3.0e7, 8.0e6]), s_star=1.0e48)


# -- the oracle ----------------------------------------------------------------------------------------------------------------
def oracle_objects(orc, hp, case):
    """(Step, State) of a case, after begin_step; a directed case's rates are in place."""
    st = orc.Step(case["mesh"], case["dr"], case["vol"], case["zred"], hp.H0, hp.Omega0, False, TEMPER_VAL, case["clumping"],
                  case["srcpos"], case["flux"], case["s_star"], case["ndens"], case["reccoef"], clumping_grid=case["clumping_grid"])
    s = orc.State(st, case["xh"], case["xhe"], case["temp"])
    orc.begin_step(s)
    if "phih" in case:
        s.phih[:], s.phihe[:], s.phiheat[:] = case["phih"], case["phihe"], case["phiheat"]
    return st, s


def _snapshot(s, conv, work, events):
    return dict(conv=int(conv), W=work.copy(), events=dict(events), xh_av=s.xh_av.copy(), xhe_av=s.xhe_av.copy(),
                xh_intermed=s.xh_intermed.copy(), xhe_intermed=s.xhe_intermed.copy(), temperature=s.temperature.copy())


def run_directed(orc, T, hp, case, dt_years, npass=NPASS):
    """`npass` global passes of the oracle on a directed case: per pass a dict of the non-converged count, the sub-steps per
    cell W, the event counts and everything the GPU test compares."""
    st, s = oracle_objects(orc, hp, case)
    out = []
    for _ in range(npass):
        conv, work, events = orc.global_pass_work(T, st, s, dt_years * YEAR)
        out.append(_snapshot(s, conv, work, events))
    return out


def run_raytraced(orc, T, hp, case, niter=RAY_ITERS, dt_years=RAY_DT):
    """`niter` outer iterations (rates to zero, all sources, global pass) of the oracle on the ray-traced case: per pass the
    dict of run_directed plus the rate grids and the columns of the source swept last."""
    st, s = oracle_objects(orc, hp, case)
    out = []
    for _ in range(niter):
        orc.pass_all_sources(T, st, s)                     # (zeroes the rate grids itself)
        rates = dict(phih=s.phih.copy(), phihe=s.phihe.copy(), phiheat=s.phiheat.copy(), sum_nbox=int(s.c.sum_nbox),
                     coldensh_out=s.coldensh_out.copy(), coldenshe_out=s.coldenshe_out.copy())
        conv, work, events = orc.global_pass_work(T, st, s, dt_years * YEAR)
        out.append(dict(_snapshot(s, conv, work, events), **rates))
    return out
