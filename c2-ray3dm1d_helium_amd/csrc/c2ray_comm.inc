// Several GPUs and the sum over ranks, behind the C ABI (included at the end of c2ray_hip.hip).
//
// The reference's only distributed strategy (SURVEY.md section 2a): every rank holds the full grid, rank r
// sweeps sources r+1, r+1+npr, ... (master_slave.F90:85), mpi_accumulate_grid_quantities
// (files_for_3D/evolve.F90:505-548) sums phih_grid, phihe_grid, phiheat, photon_loss and sum_nbox over the ranks
// with six MPI_ALLREDUCE calls through host memory, and every rank runs the global pass on the sums.
// Here a "rank" is a GPU; the six sums are ONE fp64 ncclAllReduce (RCCL, ring over xGMI) of the contiguous
// buffer [phih | phihe(0) | phihe(1) | phiheat | photon_loss(1:47) | sum_nbox], device to device -- or, cut into
// slabs of k-planes, overlapped with the rates kernel that still computes later slabs and with the chemistry of
// the slabs already summed (c2r_pass_allreduce_chemistry).
//
// Two ways to get more than one GPU, which compose:
//   * one process per GPU (MPI ranks, torch.distributed.run ranks): c2r_create + c2r_comm_init(rank, nranks, id)
//     with the id of c2r_comm_unique_id passed around by the launcher's own means (MPI_Bcast, a file, ...);
//   * one process, several GPUs: c2r_create_multi -- the returned context fans every state-setting call out to
//     all its devices, runs the passes on one host thread per device and sums with ncclCommInitAll's
//     communicators.  This is how the reference's no_mpi build drives a whole node.
// RCCL is loaded on first use (dlopen), so single-GPU users neither link nor load its 570 MB at RUN time.  At BUILD
// time the declarations of <rccl/rccl.h> are needed (types, enum values, prototypes: /opt/rocm/include/rccl on a ROCm
// installation); _build.py checks for the header and says so, INTEGRATION.md lists it among the build requirements.
#include <dlfcn.h>
#if !__has_include(<rccl/rccl.h>)
#error "libc2ray_hip needs the RCCL development header <rccl/rccl.h> (part of ROCm: /opt/rocm/include/rccl) at build time; RCCL itself is only loaded at run time, and only when a communicator is asked for"
#endif
#include <rccl/rccl.h> // types, enum values and prototypes only: the library itself is loaded with dlopen on first use

#include <mutex>
#include <thread>

namespace {

// Entry points of librccl, typed by the declarations of the header this file was compiled against.
struct Rccl {
  void *handle = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  int version = 0;
  std::string err;
};
static_assert(sizeof(ncclUniqueId) == 128, "c2r_comm_unique_id hands out 128 bytes");

void rccl_load(Rccl &R) {
  // C2R_RCCL_LIBRARY: this file and no other (an RCCL build outside the loader's path -- or the stand-in of
  // tests/fake_rccl.hip, which sums between communicators that share ONE device; c2r_comm_library says what was loaded
  // and bench.py prints it)
  const char *forced = getenv("C2R_RCCL_LIBRARY");
  if (forced && *forced) {
    R.handle = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
    if (!R.handle) {
      R.err = std::string("C2R_RCCL_LIBRARY=") + forced + ": " + dlerror();
      return;
    }
  } else {
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      R.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (R.handle) break;
    }
  }
  if (!R.handle) {
    R.err = std::string("librccl.so not found: ") + dlerror();
    return;
  }
  auto sym = [&](const char *n) {
    void *f = dlsym(R.handle, n);
    if (!f && R.err.empty()) R.err = std::string("librccl.so lacks ") + n;
    return f;
  };
  R.GetVersion = reinterpret_cast<decltype(R.GetVersion)>(sym("ncclGetVersion"));
  R.GetUniqueId = reinterpret_cast<decltype(R.GetUniqueId)>(sym("ncclGetUniqueId"));
  R.CommInitRank = reinterpret_cast<decltype(R.CommInitRank)>(sym("ncclCommInitRank"));
  R.CommInitAll = reinterpret_cast<decltype(R.CommInitAll)>(sym("ncclCommInitAll"));
  R.CommDestroy = reinterpret_cast<decltype(R.CommDestroy)>(sym("ncclCommDestroy"));
  R.CommAbort = reinterpret_cast<decltype(R.CommAbort)>(sym("ncclCommAbort"));
  R.AllReduce = reinterpret_cast<decltype(R.AllReduce)>(sym("ncclAllReduce"));
  R.GroupStart = reinterpret_cast<decltype(R.GroupStart)>(sym("ncclGroupStart"));
  R.GroupEnd = reinterpret_cast<decltype(R.GroupEnd)>(sym("ncclGroupEnd"));
  R.GetErrorString = reinterpret_cast<decltype(R.GetErrorString)>(sym("ncclGetErrorString"));
  if (!R.err.empty()) return;
  // The calls below pass ncclUniqueId by value and the enum values of the header compiled against: refuse a
  // library of another major version than that header describes (NCCL keeps its ABI within a major version).
  if (R.GetVersion(&R.version) != ncclSuccess) {
    R.err = "ncclGetVersion failed";
    return;
  }
  const int major = R.version >= 10000 ? R.version / 10000 : R.version / 1000;
  if (major != NCCL_MAJOR)
    R.err = "librccl.so reports version " + std::to_string(R.version) + ", this library was compiled against the headers of " +
            std::to_string(NCCL_VERSION_CODE) + " (another major version): refusing to call it";
}

Rccl *rccl() {
  static Rccl R;
  static std::once_flag once;
  std::call_once(once, [] { rccl_load(R); });
  return &R;
}

#define NCCLCHK(c, call)                                                                                       \
  do {                                                                                                         \
    ncclResult_t r_ = (call);                                                                                  \
    if (r_ != ncclSuccess) return fail(c, "%s failed: %s (%s:%d)", #call, rccl()->GetErrorString(r_), __FILE__, __LINE__); \
  } while (0)
// inside ncclGroupStart .. ncclGroupEnd: close the group before returning the error
#define NCCLCHK_GROUP(c, call)                                                                                 \
  do {                                                                                                         \
    ncclResult_t r_ = (call);                                                                                  \
    if (r_ != ncclSuccess) {                                                                                   \
      (void)rccl()->GroupEnd();                                                                                \
      return fail(c, "%s failed: %s (%s:%d)", #call, rccl()->GetErrorString(r_), __FILE__, __LINE__);         \
    }                                                                                                          \
  } while (0)

// all devices of a context, the leader first
std::vector<c2r_ctx *> devices_of(c2r_ctx *c) {
  std::vector<c2r_ctx *> v{c};
  v.insert(v.end(), c->replicas.begin(), c->replicas.end());
  return v;
}

// f(ctx, index) on every device of the context at once, one host thread each (the passes are host-driven:
// one thread would run the devices one after another)
template <class F>
int on_all_devices(c2r_ctx *c, F f) {
  const std::vector<c2r_ctx *> dev = devices_of(c);
  if (dev.size() == 1) return f(c, 0);
  std::vector<int> rc(dev.size(), 0);
  std::vector<std::thread> th;
  for (size_t i = 1; i < dev.size(); i++) th.emplace_back([&, i] { rc[i] = f(dev[i], (int)i); });
  rc[0] = f(dev[0], 0);
  for (auto &t : th) t.join();
  for (size_t i = 0; i < dev.size(); i++)
    if (rc[i]) {
      if (i > 0) c->err = "device " + std::to_string(dev[i]->device) + ": " + dev[i]->err;
      return rc[i];
    }
  return 0;
}

// dst[i] += src[i] (the in-process sum of replicas that share a device: rank order, deterministic)
__global__ void __launch_bounds__(BLOCK) k_add_into(double *__restrict__ dst, const double *__restrict__ src, size_t n) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) dst[i] = dst[i] + src[i];
}

// ranges of the reduction buffer that belong to cells [c0, c0+cnt): one per component that is in use
int slab_ranges(const c2r_ctx *c, size_t c0, size_t cnt, size_t off[4], size_t len[4]) {
  const int ncomp = c->isothermal ? 3 : 4; // phiheat stays zero in isothermal runs
  for (int k = 0; k < ncomp; k++) {
    off[k] = (size_t)k * c->g.ncell + c0;
    len[k] = cnt;
  }
  return ncomp;
}

// The sum over ranks of `nr` ranges of every local device's reduction buffer, queued on each device's comm
// stream (kind 1: one grouped RCCL launch per device; kind 2: through the leader's buffer).
int sum_ranges(c2r_ctx *c, int nr, const size_t *off, const size_t *len) {
  const std::vector<c2r_ctx *> dev = devices_of(c);
  if (c->comm_kind == 1) {
    Rccl *R = rccl();
    NCCLCHK(c, R->GroupStart());
    for (c2r_ctx *d : dev)
      for (int k = 0; k < nr; k++)
        NCCLCHK_GROUP(c, R->AllReduce(d->d_rates + off[k], d->d_rates + off[k], len[k], ncclFloat64, ncclSum,
                                      static_cast<ncclComm_t>(d->comm), d->comm_stream));
    NCCLCHK(c, R->GroupEnd());
  } else if (c->comm_kind == 2) {
    // every replica's stream has reached this point (events), then the leader adds the others in rank order
    // and hands the sums back
    for (size_t i = 1; i < dev.size(); i++) {
      HIPCHK(c, hipEventRecord(dev[i]->ev_comm_a, dev[i]->comm_stream));
      HIPCHK(c, hipStreamWaitEvent(c->comm_stream, dev[i]->ev_comm_a, 0));
    }
    for (size_t i = 1; i < dev.size(); i++)
      for (int k = 0; k < nr; k++) {
        const int nblk = (int)std::min<size_t>(4096, (len[k] + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL(k_add_into, dim3(nblk), dim3(BLOCK), 0, c->comm_stream, c->d_rates + off[k], dev[i]->d_rates + off[k], len[k]);
      }
    HIPCHK(c, hipGetLastError());
    for (size_t i = 1; i < dev.size(); i++)
      for (int k = 0; k < nr; k++)
        HIPCHK(c, hipMemcpyAsync(dev[i]->d_rates + off[k], c->d_rates + off[k], sizeof(double) * len[k], hipMemcpyDeviceToDevice, c->comm_stream));
    HIPCHK(c, hipEventRecord(c->ev_comm_b, c->comm_stream));
    for (size_t i = 1; i < dev.size(); i++) HIPCHK(c, hipStreamWaitEvent(dev[i]->comm_stream, c->ev_comm_b, 0));
  }
  return 0;
}

int comm_prepare(c2r_ctx *d) {
  HIPCHK(d, hipSetDevice(d->device));
  if (!d->comm_stream) HIPCHK(d, hipStreamCreateWithFlags(&d->comm_stream, hipStreamNonBlocking));
  if (!d->ev_comm_a) HIPCHK(d, hipEventCreateWithFlags(&d->ev_comm_a, hipEventDisableTiming));
  if (!d->ev_comm_b) HIPCHK(d, hipEventCreateWithFlags(&d->ev_comm_b, hipEventDisableTiming));
  return 0;
}

// summed tail of the buffer -> the host mirrors c2r_get_loss returns (photon_loss_all, sum_nbox_all)
int fetch_summed_tail(c2r_ctx *d) {
  HIPCHK(d, hipSetDevice(d->device));
  double tail[C2R_NFREQ + 1];
  HIPCHK(d, hipMemcpyAsync(tail, d->d_rates + 4 * d->g.ncell, sizeof tail, hipMemcpyDeviceToHost, d->comm_stream));
  if (sync_stream(d, d->comm_stream, "the sum over the ranks")) return 1;
  std::memcpy(d->photon_loss, tail, sizeof d->photon_loss);
  d->sum_nbox = (int)(tail[C2R_NFREQ] + 0.5);
  return 0;
}

// Fail together.  The reference's ranks meet again at the next MPI_ALLREDUCE whatever happened in a pass
// (files_for_3D/evolve.F90:177-181, :523-538) and its drop-in host ends the job with MPI_ABORT (fortran/evolve_data.F90
// stop_with).  Here an error return between the first and the last collective of an iteration would leave this
// context's communicators with sums that its peers have issued and it never will: ncclCommDestroy would then wait for
// ever, and so would the peers.  So the communicators of a context are ABORTED before such an error is returned:
// nothing of this process waits any longer, the context refuses further collective work, and the host is expected to
// exit non-zero (the launcher -- mpirun, torch.distributed.run -- then ends the other ranks; a rank that is not ended
// that way leaves its own wait through the watchdog of sync_stream, C2R_COMM_TIMEOUT_S, and aborts likewise).
void comm_abort_all(c2r_ctx *c, const std::string &why) {
  for (c2r_ctx *d : devices_of(c)) {
    if (d->comm_kind != 1) continue;
    if (d->comm) {
      (void)hipSetDevice(d->device);
      (void)rccl()->CommAbort(static_cast<ncclComm_t>(d->comm));
      d->comm = nullptr;
    }
    d->comm_broken = true;
    d->comm_broken_why = why;
  }
}

template <class F>
int with_comm_abort(c2r_ctx *c, const char *who, F body) {
  if (c->comm_kind == 1 && c->comm_broken)
    return fail(c, "%s: the communicator of this context was aborted after an earlier error (%s); make a new context", who,
                c->comm_broken_why.c_str());
  const int rc = body();
  if (rc && c->comm_kind == 1) {
    const std::string why = c->err;
    comm_abort_all(c, why);
    c->err = why + " [the RCCL communicator(s) of this context were aborted: no rank of this process waits in a sum that cannot "
                   "complete; end the job -- peers leave their own wait through the launcher or their C2R_COMM_TIMEOUT_S watchdog]";
  }
  return rc;
}

// ---- c2r_comm_selftest: the pattern of include/c2ray_hip.h ------------------------------------------------------------
// v(r, i) = (r + 1) a(i) 2^e(i); `mult` is r + 1 for what a rank contributes and n (n + 1) / 2 for the sum
__host__ __device__ inline double selftest_value(unsigned long long i, unsigned long long mult) {
  unsigned long long z = i + 0x9E3779B97F4A7C15ull; // splitmix64
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  const unsigned long long h = z ^ (z >> 31);
  const unsigned long long a = ((1ull << 29) + (h & ((1ull << 29) - 1))) | 1ull;
  const int e = (int)((h >> 32) % 121ull) - 60;
  return ldexp((double)(mult * a), e); // mult * a < 2^53: exact
}

// buf[i] = v(rank, i) for the whole buffer; resets the route's record {mismatches, lowest mismatching index}
__global__ void __launch_bounds__(BLOCK) k_selftest_fill(double *__restrict__ buf, size_t n, unsigned long long mult,
                                                         unsigned long long *__restrict__ rec) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rec[0] = 0ull;
    rec[1] = ~0ull;
  }
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) buf[i] = selftest_value(i, mult);
}

// buf[off .. off+len) against the closed form of the sum: per block one count and one lowest index, one atomic each
__global__ void __launch_bounds__(BLOCK) k_selftest_check(const double *__restrict__ buf, size_t off, size_t len,
                                                          unsigned long long mult_sum, unsigned long long *__restrict__ rec) {
  __shared__ unsigned long long s_bad[BLOCK], s_lo[BLOCK];
  unsigned long long bad = 0ull, lo = ~0ull;
  for (size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x; j < len; j += (size_t)gridDim.x * BLOCK) {
    const size_t i = off + j;
    if (!(buf[i] == selftest_value(i, mult_sum))) { // (a NaN is a mismatch)
      bad++;
      lo = lo < i ? lo : (unsigned long long)i;
    }
  }
  s_bad[threadIdx.x] = bad;
  s_lo[threadIdx.x] = lo;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_bad[threadIdx.x] += s_bad[threadIdx.x + w];
      const unsigned long long o = s_lo[threadIdx.x + w];
      if (o < s_lo[threadIdx.x]) s_lo[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_bad[0]) {
    atomicAdd(&rec[0], s_bad[0]);
    atomicMin(&rec[1], s_lo[0]);
  }
}

int selftest_grid(size_t n) { return (int)std::max<size_t>(1, std::min<size_t>(4096, (n + BLOCK - 1) / BLOCK)); }

// everything of the self-test that allocates, before its timed part
int selftest_prepare(c2r_ctx *d, int nslab) {
  HIPCHK(d, hipSetDevice(d->device));
  if (!d->d_selftest) HIPCHK(d, hipMalloc(&d->d_selftest, sizeof(unsigned long long) * 4));
  if (!d->h_selftest) HIPCHK(d, hipHostMalloc(&d->h_selftest, sizeof(unsigned long long) * 6));
  for (hipEvent_t &e : d->ev_selftest)
    if (!e) HIPCHK(d, hipEventCreate(&e));
  for (std::vector<hipEvent_t> *list : {&d->ev_slab, &d->ev_sum})
    while (list->size() < (size_t)nslab) {
      hipEvent_t e;
      HIPCHK(d, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      list->push_back(e);
    }
  return 0;
}

// the route's record and, where something mismatched, the value found at the lowest such index: through the pinned
// members of the context, behind sync_stream on the comm stream (the C2R_COMM_TIMEOUT_S watchdog covers a peer that
// never arrives)
int selftest_collect(c2r_ctx *c, const std::vector<c2r_ctx *> &dev, int route) {
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    HIPCHK(c, hipMemcpyAsync(d->h_selftest + 2 * route, d->d_selftest + 2 * route, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, d->comm_stream));
  }
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    if (sync_stream(d, d->comm_stream, "the self-test of the sum over the ranks")) { c->err = d->err; return 1; }
  }
  for (c2r_ctx *d : dev) {
    if (!d->h_selftest[2 * route]) continue;
    HIPCHK(c, hipSetDevice(d->device));
    HIPCHK(c, hipMemcpyAsync(d->h_selftest + 4 + route, d->d_rates + d->h_selftest[2 * route + 1], sizeof(double), hipMemcpyDeviceToHost, d->comm_stream));
    if (sync_stream(d, d->comm_stream, "the self-test of the sum over the ranks")) { c->err = d->err; return 1; }
  }
  return 0;
}

// c2r_get_comm_timing: the timing events of a device, made before its pass (nothing is made or recorded with timing off)
int comm_timing_prepare(c2r_ctx *d) {
  if (!d->timing) {
    d->ctm = c2r_comm_timing{};
    return 0;
  }
  for (hipEvent_t &e : d->ev_ct)
    if (!e) HIPCHK(d, hipEventCreate(&e));
  return 0;
}
int comm_timing_mark(c2r_ctx *c, c2r_ctx *d, int which) {
  if (d->timing) HIPCHK(c, hipEventRecord(d->ev_ct[which], d->comm_stream));
  return 0;
}
// ... read once the iteration's synchronisation is behind us
int comm_timing_read(c2r_ctx *c, c2r_ctx *d) {
  if (!d->timing) return 0;
  HIPCHK(c, hipSetDevice(d->device));
  float ms = 0;
  d->ctm = c2r_comm_timing{};
  d->ctm.slabs = d->pass_slabs;
  HIPCHK(c, hipEventElapsedTime(&ms, d->ev_ct[1], d->ev_ct[4]));
  d->ctm.allreduce_ms = ms;
  HIPCHK(c, hipEventElapsedTime(&ms, d->ev_ct[3], d->ev_ct[4]));
  d->ctm.tail_ms = ms;
  if (d->ct_rates_recorded) {
    // from the later of "rates complete" and "first sum released": a device whose rates were through before the host had
    // queued the first sum (a rank without sources; any rank of a tiny mesh) has waited for the host until then, not for
    // the wire -- so the exposed part lies inside [first sum released, tail complete] and never exceeds allreduce_ms
    float to_sum = 0, to_release = 0;
    HIPCHK(c, hipEventElapsedTime(&to_sum, d->ev_ct[0], d->ev_ct[2]));
    HIPCHK(c, hipEventElapsedTime(&to_release, d->ev_ct[0], d->ev_ct[1]));
    d->ctm.allreduce_exposed_ms = std::max(0.0f, to_sum - std::max(0.0f, to_release));
  }
  return 0;
}

} // namespace

extern "C" int c2r_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int c2r_create_multi(c2r_ctx **out, int ndev, const int *devices, const int mesh[3]) {
  if (!out || !devices || ndev < 1) return fail(nullptr, "c2r_create_multi: bad arguments");
  c2r_ctx *lead = nullptr;
  if (c2r_create(&lead, devices[0], mesh)) return 1;
  for (int i = 1; i < ndev; i++) {
    c2r_ctx *r = nullptr;
    if (c2r_create(&r, devices[i], mesh)) {
      c2r_destroy(lead);
      return 1;
    }
    lead->replicas.push_back(r);
  }
  *out = lead;
  return 0;
}

extern "C" int c2r_num_devices(const c2r_ctx *c) { return c ? 1 + (int)c->replicas.size() : 0; }
extern "C" int c2r_comm_nranks(const c2r_ctx *c) { return c ? c->comm_nranks : 0; }
extern "C" int c2r_comm_rank(const c2r_ctx *c) { return c ? c->comm_rank : 0; }
extern "C" int c2r_comm_kind(const c2r_ctx *c) { return c ? c->comm_kind : 0; }
extern "C" int c2r_get_timing_device(c2r_ctx *c, int idev, c2r_timing *out) {
  if (!c || !out) return 1;
  if (idev < 0 || idev > (int)c->replicas.size()) return fail(c, "c2r_get_timing_device: device %d of %d", idev, 1 + (int)c->replicas.size());
  *out = idev == 0 ? c->tm : c->replicas[(size_t)idev - 1]->tm;
  return 0;
}

extern "C" int c2r_comm_available(void) {
  Rccl *R = rccl();
  if (!R->err.empty()) return fail(nullptr, "c2r_comm_available: %s", R->err.c_str());
  return 0;
}

// Path of the library that carries the sums (dladdr of its ncclAllReduce): "" before a communicator was asked for
extern "C" int c2r_comm_library(char *out, int capacity) {
  if (!out || capacity < 1) return 1;
  out[0] = 0;
  Rccl *R = rccl();
  if (!R->err.empty()) return fail(nullptr, "c2r_comm_library: %s", R->err.c_str());
  Dl_info info;
  if (dladdr(reinterpret_cast<void *>(R->AllReduce), &info) && info.dli_fname) snprintf(out, (size_t)capacity, "%s", info.dli_fname);
  return 0;
}

extern "C" int c2r_comm_unique_id(char id[128]) {
  Rccl *R = rccl();
  if (!R->err.empty()) return fail(nullptr, "c2r_comm_unique_id: %s", R->err.c_str());
  ncclUniqueId u;
  const ncclResult_t rc = R->GetUniqueId(&u);
  if (rc != ncclSuccess) return fail(nullptr, "ncclGetUniqueId failed: %s", R->GetErrorString(rc));
  std::memcpy(id, u.internal, 128);
  return 0;
}

// c2r_comm_selftest (see the header): a known pattern through the context's own buffer, communicators, comm streams and
// events, by the routines and in the stream order of the two production routes
static int comm_selftest_body(c2r_ctx *c, int nslab, c2r_comm_selftest_report *rep) {
  const std::vector<c2r_ctx *> dev = devices_of(c);
  const unsigned long long n = (unsigned long long)c->comm_nranks, mult_sum = n * (n + 1) / 2;
  const size_t plane = (size_t)c->g.n1 * c->g.n2, ncell = c->g.ncell;
  const int ns = std::min(nslab, c->g.n3);
  rep->ranks = c->comm_nranks;
  rep->kind = c->comm_kind;
  rep->devices = (int)dev.size();
  for (c2r_ctx *d : dev) {
    if (d->pass_open) return fail(c, "c2r_comm_selftest: a pass is open (c2r_pass_sources_begin without c2r_pass_sources_end)");
    if (selftest_prepare(d, ns)) { c->err = d->err; return 1; }
    // what the test leaves in the buffer is never read: the next pass finds c2r_set_rates_to_zero's state (phiheat
    // included, which an isothermal pass would otherwise take for zero)
    d->rates_zero_pending = true;
    d->phiheat_dirty = true;
  }
  // route 0, as c2r_allreduce_rates: the whole buffer in one all-reduce
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    if (d == c) HIPCHK(c, hipEventRecord(c->ev_selftest[0], c->stream));
    hipLaunchKernelGGL(k_selftest_fill, dim3(selftest_grid(c->rates_count)), dim3(BLOCK), 0, d->stream, d->d_rates, c->rates_count,
                       (unsigned long long)d->comm_rank + 1, d->d_selftest);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(d->ev_comm_a, d->stream));
    HIPCHK(c, hipStreamWaitEvent(d->comm_stream, d->ev_comm_a, 0));
  }
  {
    const size_t off[1] = {0}, len[1] = {c->rates_count};
    if (sum_ranges(c, 1, off, len)) return 1;
  }
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    hipLaunchKernelGGL(k_selftest_check, dim3(selftest_grid(c->rates_count)), dim3(BLOCK), 0, d->comm_stream, d->d_rates, (size_t)0,
                       c->rates_count, mult_sum, d->d_selftest);
    HIPCHK(c, hipGetLastError());
    if (d == c) HIPCHK(c, hipEventRecord(c->ev_selftest[1], c->comm_stream));
  }
  rep->elements[0] = (long long)c->rates_count;
  if (selftest_collect(c, dev, 0)) return 1;
  // route 1, as c2r_pass_allreduce_chemistry: slab by slab behind the slab events, each slab's component ranges in one
  // grouped launch, the check of a slab behind the event of its sum (where production queues its chemistry), then the tail
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    if (d == c) HIPCHK(c, hipEventRecord(c->ev_selftest[2], c->stream));
    hipLaunchKernelGGL(k_selftest_fill, dim3(selftest_grid(c->rates_count)), dim3(BLOCK), 0, d->stream, d->d_rates, c->rates_count,
                       (unsigned long long)d->comm_rank + 1, d->d_selftest + 2);
    HIPCHK(c, hipGetLastError());
    for (int sidx = 0; sidx < ns; sidx++) HIPCHK(c, hipEventRecord(d->ev_slab[sidx], d->stream));
  }
  int ncomp = 0;
  for (int sidx = 0; sidx < ns; sidx++) {
    const size_t k0 = (size_t)((long long)c->g.n3 * sidx / ns), k1 = (size_t)((long long)c->g.n3 * (sidx + 1) / ns);
    size_t off[4], len[4];
    const int nr = ncomp = slab_ranges(c, plane * k0, plane * (k1 - k0), off, len);
    for (c2r_ctx *d : dev) {
      HIPCHK(c, hipSetDevice(d->device));
      HIPCHK(c, hipStreamWaitEvent(d->comm_stream, d->ev_slab[sidx], 0));
    }
    if (sum_ranges(c, nr, off, len)) return 1;
    for (c2r_ctx *d : dev) {
      HIPCHK(c, hipSetDevice(d->device));
      HIPCHK(c, hipEventRecord(d->ev_sum[sidx], d->comm_stream));
      HIPCHK(c, hipStreamWaitEvent(d->stream, d->ev_sum[sidx], 0));
      for (int k = 0; k < nr; k++)
        hipLaunchKernelGGL(k_selftest_check, dim3(selftest_grid(len[k])), dim3(BLOCK), 0, d->stream, d->d_rates, off[k], len[k], mult_sum,
                           d->d_selftest + 2);
      HIPCHK(c, hipGetLastError());
    }
  }
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    HIPCHK(c, hipEventRecord(d->ev_comm_a, d->stream));
    HIPCHK(c, hipStreamWaitEvent(d->comm_stream, d->ev_comm_a, 0));
  }
  {
    const size_t off[1] = {4 * ncell}, len[1] = {(size_t)C2R_NFREQ + 1};
    if (sum_ranges(c, 1, off, len)) return 1;
  }
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    hipLaunchKernelGGL(k_selftest_check, dim3(1), dim3(BLOCK), 0, d->comm_stream, d->d_rates, 4 * ncell, (size_t)C2R_NFREQ + 1, mult_sum,
                       d->d_selftest + 2);
    HIPCHK(c, hipGetLastError());
    if (d == c) HIPCHK(c, hipEventRecord(c->ev_selftest[3], c->comm_stream));
  }
  rep->elements[1] = (long long)((size_t)ncomp * ncell + C2R_NFREQ + 1);
  if (selftest_collect(c, dev, 1)) return 1;
  // the verdict: local to this process
  HIPCHK(c, hipSetDevice(c->device));
  for (int route = 0; route < 2; route++) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_selftest[2 * route], c->ev_selftest[2 * route + 1]));
    rep->ms[route] = ms;
  }
  const c2r_ctx *bad_dev = nullptr;
  for (int route = 0; route < 2; route++)
    for (const c2r_ctx *d : dev) {
      const unsigned long long bad = d->h_selftest[2 * route];
      rep->mismatches[route] += (long long)bad;
      if (bad && !bad_dev) {
        bad_dev = d;
        rep->bad_route = route;
        rep->bad_rank = d->comm_rank;
        rep->bad_index = (long long)d->h_selftest[2 * route + 1];
        std::memcpy(&rep->got, d->h_selftest + 4 + route, sizeof(double));
        rep->expected = selftest_value((unsigned long long)rep->bad_index, mult_sum);
      }
    }
  if (!bad_dev) return 0;
  char lib[1024] = "the in-process sum of replicas that share a device";
  if (c->comm_kind == 1) (void)c2r_comm_library(lib, (int)sizeof lib);
  unsigned long long gb, eb;
  std::memcpy(&gb, &rep->got, 8);
  std::memcpy(&eb, &rep->expected, 8);
  char msg[2048];
  snprintf(msg, sizeof msg,
           "c2r_comm_selftest: the sum over the %d ranks came back WRONG: route %d (%s), rank %d, device %d, index %lld of the "
           "reduction buffer: got %.17g (0x%016llx), expected %.17g (0x%016llx); mismatches on this process's %d device(s): %lld of "
           "%lld doubles (whole buffer), %lld of %lld (slab-wise); library: %s",
           rep->ranks, rep->bad_route, rep->bad_route == 0 ? "whole buffer, as c2r_allreduce_rates" : "slab-wise, as c2r_pass_allreduce_chemistry",
           rep->bad_rank, bad_dev->device, rep->bad_index, rep->got, gb, rep->expected, eb, rep->devices, rep->mismatches[0],
           rep->elements[0] * rep->devices, rep->mismatches[1], rep->elements[1] * rep->devices, lib);
  c->err = msg;
  return 1;
}

extern "C" int c2r_comm_selftest(c2r_ctx *c, int nslab, c2r_comm_selftest_report *rep) {
  if (!c || !rep) return 1;
  std::memset(rep, 0, sizeof *rep);
  rep->bad_route = rep->bad_rank = -1;
  rep->bad_index = -1;
  rep->ranks = 1;
  if (nslab < 1) return fail(c, "c2r_comm_selftest: nslab=%d", nslab);
  if (!c->comm_kind) {
    if (!c->replicas.empty()) return fail(c, "c2r_comm_selftest: a multi-device context needs c2r_comm_init_local or c2r_comm_init first");
    rep->devices = 1;
    return 0; // one rank: nothing is summed, nothing to check
  }
  if (c->comm_nranks > 4095)
    return fail(c, "c2r_comm_selftest: %d ranks; the pattern's sums are exact (below 2^53) for at most 4095", c->comm_nranks);
  return with_comm_abort(c, "c2r_comm_selftest", [&] { return comm_selftest_body(c, nslab, rep); });
}

// C2R_COMM_SELFTEST=1: the communicators of a context are tested before c2r_comm_init / c2r_comm_init_local hand them out
static int selftest_at_init(c2r_ctx *c, const char *who) {
  const char *on = getenv("C2R_COMM_SELFTEST");
  if (!on || atoi(on) <= 0) return 0;
  const char *env = getenv("C2R_ALLREDUCE_SLABS");
  c2r_comm_selftest_report rep;
  if (c2r_comm_selftest(c, env && atoi(env) > 0 ? atoi(env) : 4, &rep)) {
    const std::string why = c->err;
    (void)c2r_comm_destroy(c);
    c->err = std::string(who) + " (C2R_COMM_SELFTEST): " + why;
    return 1;
  }
  char lib[1024] = "none (in-process sum of replicas that share a device)";
  if (rep.kind == 1) (void)c2r_comm_library(lib, (int)sizeof lib);
  fprintf(stderr, "c2ray_hip: comm self-test ok: %d ranks, %lld + %lld doubles on each of %d device(s), %.3f + %.3f ms, library %s\n", rep.ranks,
          rep.elements[0], rep.elements[1], rep.devices, rep.ms[0], rep.ms[1], lib);
  return 0;
}

extern "C" int c2r_get_comm_timing(c2r_ctx *c, int idev, c2r_comm_timing *out) {
  if (!c || !out) return 1;
  if (idev < 0 || idev > (int)c->replicas.size()) return fail(c, "c2r_get_comm_timing: device %d of %d", idev, 1 + (int)c->replicas.size());
  *out = idev == 0 ? c->ctm : c->replicas[(size_t)idev - 1]->ctm;
  return 0;
}

// Rank `first_rank + i` of `nranks` for the i-th device of the context (one device: rank first_rank).
// The source split of c2r_evolve3d / the Fortran shim (process p of P takes sources 1 + p + i * P on its device i)
// assumes that every process drives the same number of devices, in rank order: first_rank and nranks must be
// multiples of this context's device count.
extern "C" int c2r_comm_init(c2r_ctx *c, int first_rank, int nranks, const char id[128]) {
  if (!c || !id) return 1;
  const std::vector<c2r_ctx *> dev = devices_of(c);
  const int ndev = (int)dev.size();
  if (first_rank < 0 || nranks < 1 || first_rank + ndev > nranks)
    return fail(c, "c2r_comm_init: ranks %d..%d of %d", first_rank, first_rank + ndev - 1, nranks);
  if (first_rank % ndev != 0 || nranks % ndev != 0)
    return fail(c, "c2r_comm_init: first_rank %d and nranks %d must be multiples of the context's %d devices (every process "
                "drives the same number of devices; the sources are dealt process by process)", first_rank, nranks, ndev);
  if (c->comm_kind) return fail(c, "c2r_comm_init: the context already has a communicator");
  Rccl *R = rccl();
  if (!R->err.empty()) return fail(c, "c2r_comm_init: %s", R->err.c_str());
  ncclUniqueId u;
  std::memcpy(u.internal, id, 128);
  for (c2r_ctx *d : dev)
    if (comm_prepare(d)) { c->err = d->err; return 1; }
  std::vector<ncclComm_t> comms((size_t)ndev, nullptr);
  ncclResult_t rc = R->GroupStart();
  const char *what = "ncclGroupStart";
  if (rc == ncclSuccess) {
    for (int i = 0; i < ndev && rc == ncclSuccess; i++) {
      if (hipSetDevice(dev[(size_t)i]->device) != hipSuccess) { rc = ncclUnhandledCudaError; what = "hipSetDevice"; break; }
      rc = R->CommInitRank(&comms[(size_t)i], nranks, u, first_rank + i);
      what = "ncclCommInitRank";
    }
    const ncclResult_t re = R->GroupEnd(); // always: an open group must not outlive this call
    if (rc == ncclSuccess && re != ncclSuccess) { rc = re; what = "ncclGroupEnd"; }
  }
  if (rc != ncclSuccess) {
    for (ncclComm_t cm : comms)
      if (cm) (void)R->CommAbort(cm);
    return fail(c, "c2r_comm_init: %s failed: %s", what, R->GetErrorString(rc));
  }
  for (int i = 0; i < ndev; i++) {
    dev[(size_t)i]->comm = comms[(size_t)i];
    dev[(size_t)i]->comm_kind = 1;
    dev[(size_t)i]->comm_rank = first_rank + i;
    dev[(size_t)i]->comm_nranks = nranks;
  }
  return selftest_at_init(c, "c2r_comm_init");
}

// One process, the devices of a context made by c2r_create_multi: ncclCommInitAll.  Replicas that share a
// device (a rehearsal of the multi-device logic on one GPU; RCCL refuses duplicate devices) are summed in the
// process itself.
extern "C" int c2r_comm_init_local(c2r_ctx *c) {
  if (!c) return 1;
  if (c->comm_kind) return fail(c, "c2r_comm_init_local: the context already has a communicator");
  const std::vector<c2r_ctx *> dev = devices_of(c);
  std::vector<int> ids;
  bool distinct = true;
  for (c2r_ctx *d : dev) {
    distinct = distinct && std::find(ids.begin(), ids.end(), d->device) == ids.end();
    ids.push_back(d->device);
    if (comm_prepare(d)) { c->err = d->err; return 1; }
  }
  int kind = 2;
  // C2R_COMM_SHARED_DEVICE_RCCL=1: ncclCommInitAll also for devices that repeat.  The real RCCL refuses that; the
  // stand-in of tests/fake_rccl.hip (C2R_RCCL_LIBRARY) does not, which is how the kind-1 control flow runs with
  // 2..8 ranks on a one-GPU box.
  const char *shared = getenv("C2R_COMM_SHARED_DEVICE_RCCL");
  if (distinct || (shared && atoi(shared) > 0)) {
    Rccl *R = rccl();
    if (!R->err.empty()) return fail(c, "c2r_comm_init_local: %s", R->err.c_str());
    std::vector<ncclComm_t> comms(dev.size(), nullptr);
    NCCLCHK(c, R->CommInitAll(comms.data(), (int)dev.size(), ids.data()));
    for (size_t i = 0; i < dev.size(); i++) dev[i]->comm = comms[i];
    kind = 1;
  } else {
    for (c2r_ctx *d : dev)
      if (d->device != c->device) return fail(c, "c2r_comm_init_local: devices repeat but are not all the same one");
  }
  for (size_t i = 0; i < dev.size(); i++) {
    dev[i]->comm_kind = kind;
    dev[i]->comm_rank = (int)i;
    dev[i]->comm_nranks = (int)dev.size();
  }
  return selftest_at_init(c, "c2r_comm_init_local");
}

extern "C" int c2r_comm_destroy(c2r_ctx *c) {
  if (!c) return 1;
  for (c2r_ctx *d : devices_of(c)) {
    (void)hipSetDevice(d->device);
    if (d->comm_stream && !d->comm_broken) (void)hipStreamSynchronize(d->comm_stream);
    if (d->comm_kind == 1 && d->comm) (void)rccl()->CommDestroy(static_cast<ncclComm_t>(d->comm));
    d->comm = nullptr;
    d->comm_kind = 0;
    d->comm_rank = 0;
    d->comm_nranks = 1;
    d->comm_broken = false;
    d->comm_broken_why.clear();
    d->ctm = c2r_comm_timing{};
  }
  return 0;
}

// pass_all_sources (evolve.F90:385-431): device i of the context takes the sources first + i*stride, step
// stride * (number of devices) -- with first = 1 + rank, stride = npr of an MPI host this is do_grid_static's
// distribution over all GPUs of all ranks.
extern "C" int c2r_pass_sources(c2r_ctx *c, int first, int stride) {
  if (!c) return 1;
  const int ndev = c2r_num_devices(c);
  return on_all_devices(c, [&](c2r_ctx *d, int i) { return pass_sources_one(d, first + i * stride, stride * ndev); });
}

// mpi_accumulate_grid_quantities (evolve.F90:505-548): the whole reduction buffer in one all-reduce; afterwards
// every device holds the summed rate grids and c2r_get_loss / c2r_download_rates return the summed
// photon_loss and sum_nbox.
static int allreduce_rates_body(c2r_ctx *c) {
  if (!c->comm_kind) {
    if (!c->replicas.empty()) return fail(c, "c2r_allreduce_rates: a multi-device context needs c2r_comm_init_local or c2r_comm_init first");
    return 0; // one rank: nothing to add
  }
  const std::vector<c2r_ctx *> dev = devices_of(c);
  for (c2r_ctx *d : dev) { // the pass wrote the buffer on the device's own streams
    HIPCHK(c, hipSetDevice(d->device));
    if (flush_rates_zero(d)) { c->err = d->err; return 1; }
    HIPCHK(c, hipEventRecord(d->ev_comm_a, d->stream));
    HIPCHK(c, hipStreamWaitEvent(d->comm_stream, d->ev_comm_a, 0));
  }
  const size_t off[1] = {0}, len[1] = {c->rates_count};
  if (sum_ranges(c, 1, off, len)) return 1;
  for (c2r_ctx *d : dev)
    if (fetch_summed_tail(d)) { c->err = d->err; return 1; }
  return 0;
}

extern "C" int c2r_allreduce_rates(c2r_ctx *c) {
  if (!c) return 1;
  return with_comm_abort(c, "c2r_allreduce_rates", [&] { return allreduce_rates_body(c); });
}

// evolve0D_global over the whole grid (evolve.F90:443-501), on every device of the context (replicated, as on
// the reference's ranks: all hold the same sums, all get the same fractions)
extern "C" int c2r_global_pass(c2r_ctx *c, double dt, int *conv_flag) {
  if (!c) return 1;
  // every device would apply its own un-summed share of the rates
  if (!c->replicas.empty() && !c->comm_kind)
    return fail(c, "c2r_global_pass: a multi-device context needs c2r_comm_init_local or c2r_comm_init (and the sum over its devices) first");
  std::vector<int> conv((size_t)c2r_num_devices(c), 0);
  if (on_all_devices(c, [&](c2r_ctx *d, int i) { return global_pass_one(d, dt, &conv[(size_t)i]); })) return 1;
  if (conv_flag) *conv_flag = conv[0];
  return 0;
}

// One outer iteration's pass_all_sources + mpi_accumulate_grid_quantities + global_pass with all three
// overlapped: the rates launch of a device's last batch is cut into `nslab` slabs of k-planes; slab s is summed
// over the ranks (its 3 or 4 component ranges in one grouped all-reduce on the communicator's stream) while the
// device computes the rates of slab s+1, and its chemistry is queued behind the event that marks its sum
// complete, i.e. it runs while later slabs are still on the wire.  Without a communicator this is the plain
// pass followed by the plain global pass.
// the part of one device: its pass with the rates launch of the last batch cut into slabs; `own_sums`: this
// device is the only one of its process, so its thread also queues the sums and the chemistry slab by slab
static int pass_slabs_one(c2r_ctx *d, bool own_sums, int first, int stride, int nslab, double dt) {
  if (check_ready(d, "c2r_pass_allreduce_chemistry")) return 1;
  HIPCHK(d, hipSetDevice(d->device));
  d->last_first = first;
  d->last_stride = stride;
  if (comm_timing_prepare(d)) return 1;
  if (pass_list(d, dealt_share(d, first, stride), nslab)) return 1;
  d->slab_passes++;
  // C2R_FAULT_INJECT="rank:pass" (test hook): that rank returns from its pass-th slab-wise pass with an error, after its
  // sweeps and before its share of the sums -- the failure "in the middle of a pass" that fail-together is about
  if (const char *fi = getenv("C2R_FAULT_INJECT")) {
    int r = -1;
    long long p = -1;
    if (sscanf(fi, "%d:%lld", &r, &p) == 2 && r == d->comm_rank && p == d->slab_passes)
      return fail(d, "fault injected into pass %lld of rank %d (C2R_FAULT_INJECT)", p, r);
  }
  const int n = d->pass_slabs;
  while (d->ev_sum.size() < (size_t)n) {
    hipEvent_t e;
    HIPCHK(d, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    d->ev_sum.push_back(e);
  }
  if (!own_sums) return 0;
  const size_t plane = (size_t)d->g.n1 * d->g.n2;
  for (int sidx = 0; sidx < n; sidx++) {
    const size_t c0 = plane * (size_t)d->slab_k[sidx], cnt = plane * (size_t)(d->slab_k[sidx + 1] - d->slab_k[sidx]);
    size_t off[4], len[4];
    const int nr = slab_ranges(d, c0, cnt, off, len);
    HIPCHK(d, hipStreamWaitEvent(d->comm_stream, d->ev_slab[sidx], 0));
    if (sidx == 0 && comm_timing_mark(d, d, 1)) return 1;
    if (sum_ranges(d, nr, off, len)) return 1;
    HIPCHK(d, hipEventRecord(d->ev_sum[sidx], d->comm_stream));
    if (sidx == n - 1 && comm_timing_mark(d, d, 2)) return 1;
    if (c2r_global_pass_cells(d, dt, c0, cnt, d->ev_sum[sidx])) return 1;
  }
  return 0;
}

static int pass_allreduce_chemistry_body(c2r_ctx *c, int first, int stride, int nslab, double dt, int *conv_flag) {
  const std::vector<c2r_ctx *> dev = devices_of(c);
  const int ndev = (int)dev.size();
  if (!c->comm_kind) {
    if (ndev > 1) return fail(c, "c2r_pass_allreduce_chemistry: a multi-device context needs c2r_comm_init_local or c2r_comm_init first");
    if (pass_sources_one(c, first, stride)) return 1;
    return global_pass_one(c, dt, conv_flag);
  }
  // the pass of every device (one host thread per device)
  if (on_all_devices(c, [&](c2r_ctx *d, int i) { return pass_slabs_one(d, ndev == 1, first + i * stride, stride * ndev, nslab, dt); }))
    return 1;
  if (ndev > 1) {
    // one process, several devices: this thread queues every slab's sum for all of them (one grouped launch
    // per slab) behind each device's slab event, and the slab's chemistry behind the sum
    const int n = c->pass_slabs;
    const size_t plane = (size_t)c->g.n1 * c->g.n2;
    for (int sidx = 0; sidx < n; sidx++) {
      const size_t c0 = plane * (size_t)c->slab_k[sidx], cnt = plane * (size_t)(c->slab_k[sidx + 1] - c->slab_k[sidx]);
      size_t off[4], len[4];
      const int nr = slab_ranges(c, c0, cnt, off, len);
      for (c2r_ctx *d : dev) {
        HIPCHK(c, hipSetDevice(d->device));
        HIPCHK(c, hipStreamWaitEvent(d->comm_stream, d->ev_slab[sidx], 0));
        if (sidx == 0 && comm_timing_mark(c, d, 1)) return 1;
      }
      if (sum_ranges(c, nr, off, len)) return 1;
      for (c2r_ctx *d : dev) {
        HIPCHK(c, hipSetDevice(d->device));
        HIPCHK(c, hipEventRecord(d->ev_sum[sidx], d->comm_stream));
        if (sidx == n - 1 && comm_timing_mark(c, d, 2)) return 1;
        if (c2r_global_pass_cells(d, dt, c0, cnt, d->ev_sum[sidx])) { c->err = d->err; return 1; }
      }
    }
  }
  // the tail of the buffer (photon_loss, sum_nbox) once every device's pass has been closed
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    if (pass_finish(d)) { c->err = d->err; return 1; }
    HIPCHK(c, hipEventRecord(d->ev_comm_a, d->stream));
    HIPCHK(c, hipStreamWaitEvent(d->comm_stream, d->ev_comm_a, 0));
    if (comm_timing_mark(c, d, 3)) return 1;
  }
  {
    const size_t off[1] = {4 * c->g.ncell}, len[1] = {(size_t)C2R_NFREQ + 1};
    if (sum_ranges(c, 1, off, len)) return 1;
  }
  for (c2r_ctx *d : dev) {
    HIPCHK(c, hipSetDevice(d->device));
    if (comm_timing_mark(c, d, 4)) return 1;
  }
  for (c2r_ctx *d : dev)
    if (fetch_summed_tail(d)) { c->err = d->err; return 1; }
  std::vector<int> conv((size_t)ndev, 0);
  if (on_all_devices(c, [&](c2r_ctx *d, int i) { return c2r_global_pass_finish(d, &conv[(size_t)i]); })) return 1;
  for (c2r_ctx *d : dev)
    if (comm_timing_read(c, d)) return 1;
  if (conv_flag) *conv_flag = conv[0];
  return 0;
}

extern "C" int c2r_pass_allreduce_chemistry(c2r_ctx *c, int first, int stride, int nslab, double dt, int *conv_flag) {
  if (!c) return 1;
  // (a call that is refused for its arguments has issued nothing and costs the communicator nothing)
  if (first < 1 || stride < 1 || nslab < 1) return fail(c, "c2r_pass_allreduce_chemistry: first=%d stride=%d nslab=%d", first, stride, nslab);
  return with_comm_abort(c, "c2r_pass_allreduce_chemistry",
                         [&] { return pass_allreduce_chemistry_body(c, first, stride, nslab, dt, conv_flag); });
}

// The whole convergence loop of evolve3D (evolve.F90:147-217) in one call; with a communicator the rate grids
// are summed over the ranks in every iteration.
extern "C" int c2r_evolve3d(c2r_ctx *c, double dt, int *niter_out, int *conv_flags_out, int cap) {
  if (!c) return 1;
  if (check_ready(c, "c2r_evolve3d")) return 1;
  if (!c->replicas.empty() && !c->comm_kind)
    return fail(c, "c2r_evolve3d: a multi-device context needs c2r_comm_init_local or c2r_comm_init first");
  if (c2r_begin_step(c)) return 1;
  int niter = 0;
  const Grid g = c->g;
  int conv_flag = (int)g.ncell;
  const int conv_criterion = std::min((int)(convergence_fraction * g.n1 * g.n2 * g.n3), c->nsrc + c->nplane); // evolve.F90:147 (a plane counts as a source)
  const int ndev = c2r_num_devices(c);
  for (;;) {
    if (conv_flag < conv_criterion && niter > 1) { // evolve.F90:163
      if (c2r_end_step(c)) return 1;
      break;
    } else if (niter > 500) {
      break;
    }
    niter++;
    if (c2r_set_rates_to_zero(c)) return 1;
    if (c->comm_kind) {
      // this context's devices are ranks comm_rank .. comm_rank + ndev - 1 of comm_nranks: process
      // comm_rank / ndev of comm_nranks / ndev, device i of it takes sources 1 + process + i * processes, ...
      const char *env = getenv("C2R_ALLREDUCE_SLABS");
      const int nslab = env && atoi(env) > 0 ? atoi(env) : 4;
      if (c2r_pass_allreduce_chemistry(c, 1 + c->comm_rank / ndev, std::max(1, c->comm_nranks / ndev), nslab, dt, &conv_flag)) return 1;
    } else {
      if (c->nsrc + c->nplane > 0 && c2r_pass_sources(c, 1, 1)) return 1;
      if (c2r_global_pass(c, dt, &conv_flag)) return 1;
    }
    if (conv_flags_out && niter <= cap) conv_flags_out[niter - 1] = conv_flag;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (niter_out) *niter_out = niter;
  return 0;
}

// One outer iteration with everything the host loop reports about it (see the header): the pass, the sum over the
// ranks, the global pass and the grid reductions in one queue, one synchronisation.
extern "C" int c2r_iteration(c2r_ctx *c, int first, int stride, int nslab, double dt, c2r_iteration_report *rep) {
  if (!c || !rep) return 1;
  c->want_iter_stats = true; // the first device's global pass is followed by k_iter_stats (all devices hold the same state)
  int conv = 0;
  const int rc = c2r_pass_allreduce_chemistry(c, first, stride, nslab, dt, &conv);
  c->want_iter_stats = false;
  if (rc) return rc;
  rep->conv_flag = conv;
  std::memcpy(rep->photon_loss, c->photon_loss, sizeof rep->photon_loss);
  rep->sum_nbox = c->sum_nbox;
  const double *h = c->h_iter;
  const double nc = (double)c->g.ncell;
  // h0 = sum*vol*(1-abu_he) ... (photonstatistics.f90:139-143), as c2r_state_sums
  rep->sums_intermed[0] = h[0] * c->sc.vol * (1.0 - abu_he);
  rep->sums_intermed[1] = h[1] * c->sc.vol * (1.0 - abu_he);
  rep->sums_intermed[2] = h[2] * c->sc.vol * abu_he;
  rep->sums_intermed[3] = h[3] * c->sc.vol * abu_he;
  rep->sums_intermed[4] = h[4] * c->sc.vol * abu_he;
  for (int n = 0; n < 5; n++) rep->means_intermed[n] = h[5 + n] / nc;                 // as c2r_fraction_means
  for (int n = 0; n < 3; n++) rep->total_rates[n] = h[10 + n] * c->sc.vol * dt;       // photonstatistics.f90:199-201
  rep->minima_av[0] = h[ITER_NV];
  rep->minima_av[1] = h[ITER_NV + 1];
  std::memcpy(rep->reccoef, h + ITER_NV + 2, sizeof rep->reccoef);
  return 0;
}
