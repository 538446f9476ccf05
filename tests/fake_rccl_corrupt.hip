// TEST INFRASTRUCTURE ONLY (tests/).  Not part of the product; bench.py never loads it.
//
// A stand-in for librccl that LIES: the one-device stand-in of fake_rccl.hip (included below with its entry points renamed,
// every call is carried to it unchanged) plus, selected by the environment variable FAKE_RCCL_CORRUPT, a falsification of the
// DATA an all-reduce returns -- what c2r_comm_selftest (csrc/c2ray_comm.inc) exists to catch:
//
//   bitflip:R:K:I   after the K-th (1-based) all-reduce issued on rank R's communicator, the lowest mantissa bit of element I
//                   of that call's receive range on rank R is flipped
//   fp32            every element of every receive range is rounded through float
//   stale:R         rank R's receive range keeps what it held before the call (copied aside on the caller's stream before the
//                   call is forwarded, copied back afterwards: the product sums in place)
//
// The falsifying work is queued on the caller's stream AFTER the stand-in has made that stream wait for the sum: right after
// a lone ncclAllReduce, at ncclGroupEnd for calls inside a group (the stand-in only makes the streams wait there).  Unset:
// fully transparent.  It produces wrong numbers and error returns, never a hang, a fault or an abort signal.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // the entry points under their own names, declared before the stand-in's definitions are renamed

#define ncclGetVersion inner_ncclGetVersion
#define ncclGetUniqueId inner_ncclGetUniqueId
#define ncclCommInitAll inner_ncclCommInitAll
#define ncclCommInitRank inner_ncclCommInitRank
#define ncclAllReduce inner_ncclAllReduce
#define ncclGroupStart inner_ncclGroupStart
#define ncclGroupEnd inner_ncclGroupEnd
#define ncclCommDestroy inner_ncclCommDestroy
#define ncclCommAbort inner_ncclCommAbort
#define ncclGetErrorString inner_ncclGetErrorString
#define fake_rccl_stats inner_fake_rccl_stats
#include "fake_rccl.hip"
#undef ncclGetVersion
#undef ncclGetUniqueId
#undef ncclCommInitAll
#undef ncclCommInitRank
#undef ncclAllReduce
#undef ncclGroupStart
#undef ncclGroupEnd
#undef ncclCommDestroy
#undef ncclCommAbort
#undef ncclGetErrorString
#undef fake_rccl_stats

#include <cstdio>
#include <utility>

namespace {

enum { LIE_NONE = 0, LIE_BITFLIP, LIE_FP32, LIE_STALE };
struct Lie {
  int kind = LIE_NONE, rank = -1;
  unsigned long long call = 0;
  size_t index = 0;
};

Lie parse_lie() {
  Lie l;
  const char *e = getenv("FAKE_RCCL_CORRUPT");
  if (!e || !*e) return l;
  unsigned long long k = 0, i = 0;
  int r = -1;
  if (sscanf(e, "bitflip:%d:%llu:%llu", &r, &k, &i) == 3) {
    l.kind = LIE_BITFLIP;
    l.rank = r;
    l.call = k;
    l.index = (size_t)i;
  } else if (std::strcmp(e, "fp32") == 0) {
    l.kind = LIE_FP32;
  } else if (sscanf(e, "stale:%d", &r) == 1) {
    l.kind = LIE_STALE;
    l.rank = r;
  } else {
    fprintf(stderr, "fake_rccl_corrupt: FAKE_RCCL_CORRUPT=%s not understood (bitflip:R:K:I, fp32, stale:R): no corruption\n", e);
  }
  return l;
}
const Lie &lie() {
  static const Lie l = parse_lie();
  return l;
}

// what the wrapper knows of a communicator (the stand-in's Comm is private): its rank, from ncclCommInitRank's argument or
// ncclCommInitAll's index, the all-reduce calls issued on it, and the buffers stale:R copies aside into
struct Info {
  int rank = 0;
  unsigned long long calls = 0;
  std::vector<std::pair<double *, size_t>> stash; // per position in a group; never freed while copies may be queued
};
std::mutex w_m;
std::map<ncclComm_t, Info> w_info;

struct Fix {
  int kind;
  double *recv;
  size_t count, index;
  double *stash;
  hipStream_t stream;
};
thread_local int w_depth = 0;
thread_local std::vector<Fix> w_fix;

__global__ void k_flip_lowest_bit(double *p) {
  unsigned long long *q = reinterpret_cast<unsigned long long *>(p);
  *q = *q ^ 1ull;
}
__global__ void __launch_bounds__(256) k_through_float(double *p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = (double)(float)p[i];
}

ncclResult_t apply(const Fix &f) {
  if (f.kind == LIE_BITFLIP) {
    hipLaunchKernelGGL(k_flip_lowest_bit, dim3(1), dim3(1), 0, f.stream, f.recv + f.index);
  } else if (f.kind == LIE_FP32 && f.count > 0) {
    const int nblk = (int)std::min<size_t>(8192, (f.count + 255) / 256);
    hipLaunchKernelGGL(k_through_float, dim3(nblk), dim3(256), 0, f.stream, f.recv, f.count);
  } else if (f.kind == LIE_STALE && f.count > 0) {
    if (hipMemcpyAsync(f.recv, f.stash, sizeof(double) * f.count, hipMemcpyDeviceToDevice, f.stream) != hipSuccess) return ncclUnhandledCudaError;
  }
  return hipGetLastError() == hipSuccess ? ncclSuccess : ncclUnhandledCudaError;
}

} // namespace

extern "C" {

ncclResult_t ncclGetVersion(int *version) { return inner_ncclGetVersion(version); }
ncclResult_t ncclGetUniqueId(ncclUniqueId *id) { return inner_ncclGetUniqueId(id); }
const char *ncclGetErrorString(ncclResult_t r) { return inner_ncclGetErrorString(r); }
void fake_rccl_stats(long long out[4]) { inner_fake_rccl_stats(out); }

ncclResult_t ncclCommInitAll(ncclComm_t *comms, int ndev, const int *devlist) {
  const ncclResult_t rc = inner_ncclCommInitAll(comms, ndev, devlist);
  if (rc == ncclSuccess) {
    std::lock_guard<std::mutex> lk(w_m);
    for (int i = 0; i < ndev; i++) w_info[comms[i]].rank = i;
  }
  return rc;
}

ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank) {
  const ncclResult_t rc = inner_ncclCommInitRank(comm, nranks, id, rank);
  if (rc == ncclSuccess && comm && *comm) {
    std::lock_guard<std::mutex> lk(w_m);
    w_info[*comm].rank = rank;
  }
  return rc;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  {
    std::lock_guard<std::mutex> lk(w_m);
    w_info.erase(comm);
  }
  return inner_ncclCommDestroy(comm);
}

ncclResult_t ncclCommAbort(ncclComm_t comm) {
  {
    std::lock_guard<std::mutex> lk(w_m);
    w_info.erase(comm);
  }
  return inner_ncclCommAbort(comm);
}

ncclResult_t ncclAllReduce(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                           hipStream_t stream) {
  const Lie &l = lie();
  Fix f{LIE_NONE, static_cast<double *>(recvbuff), count, 0, nullptr, stream};
  if (l.kind != LIE_NONE && recvbuff && datatype == ncclFloat64) {
    std::lock_guard<std::mutex> lk(w_m);
    auto it = w_info.find(comm);
    if (it != w_info.end()) {
      Info &info = it->second;
      const unsigned long long k = ++info.calls;
      if (l.kind == LIE_FP32) {
        f.kind = LIE_FP32;
      } else if (l.kind == LIE_BITFLIP && info.rank == l.rank && k == l.call && l.index < count) {
        f.kind = LIE_BITFLIP;
        f.index = l.index;
      } else if (l.kind == LIE_STALE && info.rank == l.rank && count > 0) {
        const size_t slot = w_depth > 0 ? w_fix.size() : 0;
        if (info.stash.size() <= slot) info.stash.resize(slot + 1, {nullptr, 0});
        if (info.stash[slot].second < count) { // (the smaller one is leaked: a copy out of it may still be queued)
          if (hipMalloc(&info.stash[slot].first, sizeof(double) * count) != hipSuccess) return ncclUnhandledCudaError;
          info.stash[slot].second = count;
        }
        f.kind = LIE_STALE;
        f.stash = info.stash[slot].first;
        if (hipMemcpyAsync(f.stash, recvbuff, sizeof(double) * count, hipMemcpyDeviceToDevice, stream) != hipSuccess) return ncclUnhandledCudaError;
      }
    }
  }
  const ncclResult_t rc = inner_ncclAllReduce(sendbuff, recvbuff, count, datatype, op, comm, stream);
  if (rc != ncclSuccess || f.kind == LIE_NONE) return rc;
  if (w_depth > 0) {
    w_fix.push_back(f);
    return rc;
  }
  return apply(f);
}

ncclResult_t ncclGroupStart(void) {
  w_depth++;
  return inner_ncclGroupStart();
}

ncclResult_t ncclGroupEnd(void) {
  ncclResult_t rc = inner_ncclGroupEnd();
  if (w_depth > 0 && --w_depth > 0) return rc;
  std::vector<Fix> list;
  list.swap(w_fix);
  if (rc != ncclSuccess) return rc; // nothing was summed: nothing to falsify
  for (const Fix &f : list) {
    const ncclResult_t r = apply(f);
    if (rc == ncclSuccess) rc = r;
  }
  return rc;
}

} // extern "C"
