// exp, log10 and pow that return, bit for bit, what the reference's own libm returns.
//
// The reference (flang build, dynamically linked) gets exp, log10 and ** from glibc 2.35's libm on
// x86-64; on every CPU with FMA+AVX2 its ifunc resolvers pick __exp_fma, __log_fma and __pow_fma
// (ARM optimized-routines' exp.c / log.c / pow.c compiled with -mfma, so GCC fused many a*b+c);
// log10 is the generic fdlibm __ieee754_log10 wrapper around that log.  evolve3D's outer iteration
// amplifies a last-bit difference in any of these to the per-cent level in ionisation-front cells
// (DESIGN.md "Conditioning"), and the device libm (ocml) differs from glibc in 1-23 % of calls
// (tests/test_gpu_math.py).  So the functions below restate the three routines operation by
// operation, with an explicit fma() exactly where the x86 build has a fused instruction and
// separate roundings everywhere else (the file must be compiled with -ffp-contract=off).
// Tables: csrc/c2ray_math_tables.hpp (generated, data only).
//
// Provenance and licence: this is third-party arithmetic, not the reference's.  The algorithms and coefficient
// tables are those of glibc 2.35's sysdeps/ieee754/dbl-64/e_exp.c, e_log.c, e_pow.c (from ARM's
// optimized-routines; Copyright (C) 2018-2022 Free Software Foundation, Inc., originally Copyright (c) 2018 Arm
// Ltd., MIT) and e_log10.c (fdlibm; Copyright (C) 1993 Sun Microsystems, Inc., "permission to use, copy, modify,
// and distribute this software is freely granted, provided that this notice is preserved"), distributed with
// glibc under the GNU Lesser General Public License v2.1 or later.  The restatement below is written from the
// published algorithm and the disassembly of the image's libm.so.6; the tables in c2ray_math_tables.hpp are
// data lifted from that binary by tools/extract_glibc_math_tables.py.  A redistributor must honour LGPL-2.1+
// for this file and its tables.
//
// Domain: finite, positive, normal arguments as they occur on the hot path; anything else (zero,
// negative, subnormal, inf, nan, |y| < 2^-65 or >= 2^63 in pow) is forwarded to the platform libm.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define C2R_MHD __host__ __device__ __forceinline__
#else
#define C2R_MHD inline
#endif

namespace c2r {
namespace gm {

#define C2R_TAB static const
#define C2R_TN(n) h_##n
#include "c2ray_math_tables.hpp"
#undef C2R_TAB
#undef C2R_TN
#if defined(__HIPCC__)
#define C2R_TAB static __device__ const
#define C2R_TN(n) d_##n
#include "c2ray_math_tables.hpp"
#undef C2R_TAB
#undef C2R_TN
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define GMT(n) d_##n
#else
#define GMT(n) h_##n
#endif

C2R_MHD uint64_t asuint64(double x) { return __builtin_bit_cast(uint64_t, x); }
C2R_MHD double asdouble(uint64_t u) { return __builtin_bit_cast(double, u); }
C2R_MHD double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
// a*k + c for two literal constants k and c.  Inside a divergent branch the compiler turns such an fma into
// "copy c, then v_fmac" (one extra VALU instruction per polynomial coefficient pair); spelled out, it is the
// three-address v_fma_f64 with k in scalar registers and c in a vector register that lives across the loop.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double fma_kc(double a, double k, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(k), "v"(c));
  return d;
}
#else
C2R_MHD double fma_kc(double a, double k, double c) { return __builtin_fma(a, k, c); }
#endif

// ---- log: __log_fma ---------------------------------------------------------------------------
// the branch of __log_fma for 1 - 0x1p-4 <= x < 1 + 0x1.09p-4 (precondition)
C2R_MHD double log_near1(double x) {
  const double *B = GMT(log_hdr) + 7;
  // (glibc returns 0 for x == 1 up front; with r == 0 every term below is +0 in round-to-nearest,
  // so the shortcut changes nothing and is left out)
  const double r = x - 1.0;
  const double u1 = fma_kc(r, B[2], B[1]);
  const double u2 = fma_kc(r, B[5], B[4]);
  const double r2 = r * r;
  const double u3 = fma_kc(r, B[8], B[7]);
  const double v1 = fma_(r2, B[3], u1);
  const double v2 = fma_(r2, B[6], u2);
  const double r3 = r * r2;
  double v3 = fma_(r2, B[9], u3);
  v3 = fma_(r3, B[10], v3);
  const double w2 = fma_(v3, r3, v2);
  const double P = fma_(w2, r3, v1);
  const double t = fma_(r, 0x1p27, r);
  const double rhi = fma_(-0x1p27, r, t);
  const double rhi2 = rhi * rhi;
  const double rlo = r - rhi;
  const double hi = fma_(rhi2, B[0], r);
  const double lo = fma_(rhi2, B[0], r - hi);
  const double lo2 = fma_(B[0] * rlo, r + rhi, lo);
  const double y = fma_(P, r3, lo2);
  return hi + y;
}
// precondition: x finite, positive, normal
C2R_MHD double log_core(double x) {
  const double *H = GMT(log_hdr);
  const double Ln2hi = H[0], Ln2lo = H[1];
  const double *A = H + 2;
  const uint64_t ix = asuint64(x);
  const uint64_t LO = 0x3FEE000000000000ULL; // asuint64(1.0 - 0x1p-4)
  const uint64_t HI = 0x3FF1090000000000ULL; // asuint64(1.0 + 0x1.09p-4)
  if (ix - LO < HI - LO) return log_near1(x);
  const uint64_t tmp = ix - 0x3FE6000000000000ULL; // OFF
  const int i = (int)((tmp >> 45) & 127);
  const int k = (int)((int64_t)tmp >> 52);
  const uint64_t iz = ix - (tmp & 0xFFF0000000000000ULL);
  const double invc = GMT(log_tab)[2 * i], logc = GMT(log_tab)[2 * i + 1];
  const double z = asdouble(iz);
  const double kd = (double)k;
  const double r = fma_(z, invc, -1.0);
  const double w = fma_(kd, Ln2hi, logc);
  const double t1 = fma_(r, A[2], A[1]);
  const double hi = r + w;
  const double r2 = r * r;
  double lo = (w - hi) + r;
  lo = fma_(kd, Ln2lo, lo);
  const double r3 = r * r2;
  const double t2 = fma_(r, A[4], A[3]);
  const double s = fma_(r2, A[0], lo);
  const double p = fma_(t2, r2, t1);
  const double q = fma_(r3, p, s);
  return q + hi;
}

// ---- log10: __ieee754_log10 (sysdeps/ieee754/dbl-64/e_log10.c, generic build, no fma) ----------
C2R_MHD double log10_(double x) {
  uint64_t ix = asuint64(x);
  const double ivln10 = asdouble(0x3FDBCB7B1526E50EULL);
  const double log10_2hi = asdouble(0x3FD34413509F6000ULL);
  const double log10_2lo = asdouble(0x3D59FEF311F12B36ULL);
  int k = 0;
  if (ix - 0x0010000000000000ULL >= 0x7FF0000000000000ULL - 0x0010000000000000ULL) {
    // e_log10.c: x < 2^-1022, or inf / nan
    if ((ix << 1) == 0) return -0x1p54 / fabs(x);              // log(+-0) = -inf
    if ((int64_t)ix < 0) return (x - x) / (x - x);             // log(-#) = NaN
    if (ix >= 0x7FF0000000000000ULL) return x + x;             // inf, nan
    k = -54;                                                   // subnormal: scale up
    ix = asuint64(x * 0x1p54);
  }
  k += (int)(ix >> 52) - 1023;
  const int i = k < 0 ? 1 : 0;
  const uint64_t hx = (ix & 0x000FFFFFFFFFFFFFULL) | ((uint64_t)(0x3ff - i) << 52);
  const double y = (double)(k + i);
  const double z = y * log10_2lo + ivln10 * log_core(asdouble(hx));
  return z + y * log10_2hi;
}

// log10 for arguments known to be positive and normal (optical depths clamped to >= 1e-20,
// temperatures): the same operations as log10_/log_core, with the 64-bit integer bookkeeping done
// on the high 32-bit word (every constant involved has a zero low word, so this is exact) and
// without the out-of-domain branch.  Bit-identical to log10_ (tests/test_math_host.py).
// The routine comes in pieces so that a caller with two arguments (the optical depths at the two faces of a
// cell) can run both table-path evaluations as one straight line -- their table loads and dependent fma chains
// overlap -- and visit the polynomial path of __log_fma (arguments within [1-2^-4, 1+0x1.09p-4), one in ten)
// only when some lane needs it.
struct Log10Arg {
  uint32_t hx, lo; // x' = x scaled by a power of two into [0.5, 2): high and low word
  int ky;          // the power of two taken out (k + i of e_log10.c)
};
C2R_MHD Log10Arg log10_split(double x) { // x positive, normal, finite
  const uint64_t ix = asuint64(x);
  const uint32_t hi = (uint32_t)(ix >> 32);
  Log10Arg a;
  a.lo = (uint32_t)ix;
  const int k = (int)(hi >> 20) - 1023;
  const int i = (int)((uint32_t)k >> 31);
  a.ky = k + i;
  // (hi & 0xFFFFF) | (0x3ff - i) << 20: the sign bit is clear, so taking k + i out of the exponent field is a
  // plain subtraction.  (Round 4 tried the other end -- mask the mantissa, select the exponent field of [1, 2) or
  // [0.5, 1), and-or, subtract, shift: five operations on paper, seven in the compiler's hands -- and kept this.)
  a.hx = hi - ((uint32_t)a.ky << 20);
  return a;
}
C2R_MHD bool log10_near1(const Log10Arg &a) { return a.hx - 0x3FEE0000u < 0x00030900u; }
C2R_MHD double log10_arg_value(const Log10Arg &a) { return asdouble(((uint64_t)a.hx << 32) | a.lo); }
// The two polynomial coefficients of the table path that enter as the ADDEND of a three-address fma (fma_kc) must be
// in vector registers; left to itself the compiler builds them anew in every band iteration (two s_mov and a
// v_mov_b64 each).  A kernel that evaluates many logs makes them once (pin_log_constants: opaque to the
// optimiser, so they stay where they are) and hands them down.
struct LogPins {
  double a1, a3;
};
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ LogPins pin_log_constants() {
  const double *A = GMT(log_hdr) + 2;
  LogPins p;
  asm volatile("v_mov_b64 %0, %1" : "=v"(p.a1) : "s"(A[1]));
  asm volatile("v_mov_b64 %0, %1" : "=v"(p.a3) : "s"(A[3]));
  return p;
}
#else
inline LogPins pin_log_constants() {
  const double *A = GMT(log_hdr) + 2;
  return LogPins{A[1], A[3]};
}
#endif
// the table path of __log_fma on x'; `tab` = log_tab (invc, logc pairs), wherever the caller keeps it
C2R_MHD double log_table_path(const Log10Arg &a, const double *tab, const LogPins *pins = nullptr) {
  const double *H = GMT(log_hdr);
  const double Ln2hi = H[0], Ln2lo = H[1];
  const double *A = H + 2;
  const double A1 = pins ? pins->a1 : A[1], A3 = pins ? pins->a3 : A[3];
  const uint32_t th = a.hx - 0x3FE60000u;
  // entry i = (th >> 13) & 127 of 16-byte (invc, logc) pairs: its byte offset in two operations
  const uint32_t off = (th >> 9) & 0x7F0u;
  const int k2 = (int)th >> 20;
  const uint32_t izh = a.hx - (th & 0xFFF00000u);
  const double z = asdouble(((uint64_t)izh << 32) | a.lo);
  const double *e = (const double *)((const char *)tab + off);
  const double invc = e[0], logc = e[1];
  const double kd = (double)k2;
  const double r = fma_(z, invc, -1.0);
  const double w = fma_(kd, Ln2hi, logc);
  const double t1 = fma_kc(r, A[2], A1);
  const double hi_ = r + w;
  const double r2 = r * r;
  double lo_ = (w - hi_) + r;
  lo_ = fma_(kd, Ln2lo, lo_);
  const double r3 = r * r2;
  const double t2 = fma_kc(r, A[4], A3);
  const double s_ = fma_(r2, A[0], lo_);
  const double p_ = fma_(t2, r2, t1);
  const double q_ = fma_(r3, p_, s_);
  return q_ + hi_;
}
// The same table path with the power of two that __log_fma takes out of x' folded into the table.  x' lies in
// [0.5, 2), so that power is k in {-1, 0, 1} and, with the 128 intervals of invc / logc, there are 256 cases,
// numbered E = (hx - 0x3FE00000) >> 13: an entry holds invc, w = fma(k, Ln2hi, logc), c = k * Ln2lo (exact) and k << 20.
// Against log_table_path this saves, per logarithm, the conversion of k, the fma that makes w and three of the integer
// operations that find k, the interval and z -- the same bits (fma(k, Ln2lo, lo) == lo + k * Ln2lo for these k).
struct LogEntry {
  double invc, w, c;
  uint32_t kshift, pad;
};
C2R_MHD LogEntry make_log_entry(int E) { // E in [0, 256)
  const double *H = GMT(log_hdr);
  const int d = E - 0x30;
  const int i = d & 127, k = d >> 7; // arithmetic shift: -1, 0, 1
  const double kd = (double)k;
  LogEntry e;
  e.invc = GMT(log_tab)[2 * i];
  e.w = fma_(kd, H[0], GMT(log_tab)[2 * i + 1]);
  e.c = kd * H[1];
  e.kshift = (uint32_t)k << 20;
  e.pad = 0;
  return e;
}
C2R_MHD double log_table_path4(const Log10Arg &a, const LogEntry *tab, const LogPins *pins = nullptr) {
  const double *A = GMT(log_hdr) + 2;
  const double A1 = pins ? pins->a1 : A[1], A3 = pins ? pins->a3 : A[3];
  const uint32_t T = a.hx - 0x3FE00000u;  // [0, 0x200000)
  const uint32_t off = (T >> 8) & 0x1FE0u; // entry T >> 13 of 32-byte entries
  const LogEntry *e = (const LogEntry *)((const char *)tab + off);
  const double invc = e->invc, w = e->w, c = e->c;
  const uint32_t izh = a.hx - e->kshift;
  const double z = asdouble(((uint64_t)izh << 32) | a.lo);
  const double r = fma_(z, invc, -1.0);
  const double t1 = fma_kc(r, A[2], A1);
  const double hi_ = r + w;
  const double r2 = r * r;
  double lo_ = (w - hi_) + r;
  lo_ = lo_ + c;
  const double r3 = r * r2;
  const double t2 = fma_kc(r, A[4], A3);
  const double s_ = fma_(r2, A[0], lo_);
  const double p_ = fma_(t2, r2, t1);
  const double q_ = fma_(r3, p_, s_);
  return q_ + hi_;
}
// __ieee754_log10's tail: log10(x) from log(x') and the power of two
C2R_MHD double log10_finish(const Log10Arg &a, double lg) {
  const double ivln10 = asdouble(0x3FDBCB7B1526E50EULL);
  const double log10_2hi = asdouble(0x3FD34413509F6000ULL);
  const double log10_2lo = asdouble(0x3D59FEF311F12B36ULL);
  const double y = (double)a.ky;
  const double zz = y * log10_2lo + ivln10 * lg;
  return zz + y * log10_2hi;
}
// The same tail with its exponent terms tabulated.  y = (double)ky and the two products y*log10_2lo, y*log10_2hi depend on
// the integer ky alone: a table indexed by ky holds the pair, filled by the very multiplications it replaces
// (make_log10_exp), and the tail is left with its two additions and the product ivln10*lg -- no fma, two roundings each,
// as the generic build of e_log10.c has them.  ky of a positive normal double that is at least 1e-20 lies in [-66, 1023];
// the table covers [-67, 1024], so that +inf (ky = 1024, which max(tau, 1e-20) lets through) reads an entry as well.
struct Log10Exp {
  double ylo, yhi; // y*log10_2lo, y*log10_2hi
};
constexpr int LOG10_KY_LO = -67, LOG10_KY_HI = 1024, LOG10_NEXP = LOG10_KY_HI - LOG10_KY_LO + 1;
C2R_MHD Log10Exp make_log10_exp(int ky) {
  const double log10_2hi = asdouble(0x3FD34413509F6000ULL);
  const double log10_2lo = asdouble(0x3D59FEF311F12B36ULL);
  const double y = (double)ky;
  Log10Exp e;
  e.ylo = y * log10_2lo;
  e.yhi = y * log10_2hi;
  return e;
}
// `xt`: entry 0 is ky = LOG10_KY_LO; precondition LOG10_KY_LO <= a.ky <= LOG10_KY_HI
C2R_MHD double log10_finish(const Log10Arg &a, double lg, const Log10Exp *xt) {
  const double ivln10 = asdouble(0x3FDBCB7B1526E50EULL);
  const Log10Exp *e = (const Log10Exp *)((const char *)xt + ((uint32_t)(a.ky - LOG10_KY_LO) << 4));
  const double ylo = e->ylo, yhi = e->yhi;
  const double zz = ylo + ivln10 * lg;
  return zz + yhi;
}
// both tables of a kernel that keeps them in LDS: a type of its own, by which tau_table_positions chooses this tail
struct LogEntryExp {
  const LogEntry *tab;
  const Log10Exp *exp;
};
// The isothermal one-SED k_rates with all axes periodic takes two more steps out of the integer bookkeeping of a logarithm
// (everything from here to LogFoldExp; no other kernel uses it).
// 1. The power of two folded into the reciprocal.  log_table_path4 uses z = x' * 2^-k (k in {-1, 0, 1}, LogEntry::kshift) in
//    one place, r = fma(z, invc, -1).  invc * 2^-k is exact, so fma(x', invc * 2^-k, -1) is the same real number rounded
//    once: the same bits, without kshift, its read and the subtraction.  A LogFold entry holds {invc * 2^-k, w, c} at the
//    pitch of LogEntry (the index arithmetic stays), read as two pieces: {invc, w} and c (with the limit of 3. behind it).
// 2. hx by a select, and the exponent table's offset from the same subtraction.  hx of log10_split is the mantissa of x
//    under the exponent field of [0.5, 1) for x < 1 and of [1, 2) otherwise; hi - hx is then ky << 20, and its arithmetic
//    shift by 16 the byte offset ky << 4 into the exponent table, counted from the entry of ky = 0.  ky itself is not formed.
// 3. The near-1 test from the table.  log10_near1's window [0x3FEE0000, 0x3FF10900) of hx starts on the boundary of entry 112
//    and ends inside entry 136, so a limit per entry -- 0 outside the window, all ones for the entries wholly inside it,
//    the window's end for entry 136 -- makes the test hx < lim: one compare, without the subtraction.  The limit stands in
//    the entry's spare bytes behind c and is read with it.
struct alignas(16) LogFold {
  double invc, w, c; // invc * 2^-k; w and c as in LogEntry
  uint32_t lim, pad; // hx is within log10_near1's window if and only if hx < lim
};
static_assert(sizeof(LogFold) == 32, "LogFold: the pitch of LogEntry");
constexpr uint32_t LOG_NEAR1_LO = 0x3FEE0000u, LOG_NEAR1_HI = 0x3FF10900u; // log10_near1's window of hx
constexpr int LOG_NEAR1_E0 = (int)((LOG_NEAR1_LO - 0x3FE00000u) >> 13), LOG_NEAR1_E1 = (int)((LOG_NEAR1_HI - 0x3FE00000u) >> 13);
static_assert(LOG_NEAR1_LO == 0x3FE00000u + ((uint32_t)LOG_NEAR1_E0 << 13) && LOG_NEAR1_E0 == 112 && LOG_NEAR1_E1 == 136,
              "LogFold::lim: the window starts with an entry");
C2R_MHD LogFold make_log_fold(int E) { // E in [0, 256)
  const LogEntry e = make_log_entry(E);
  const int k = (E - 0x30) >> 7; // as make_log_entry has it
  LogFold f;
  f.invc = e.invc * (k < 0 ? 2.0 : (k > 0 ? 0.5 : 1.0)); // exact
  f.w = e.w;
  f.c = e.c;
  f.lim = E < LOG_NEAR1_E0 || E > LOG_NEAR1_E1 ? 0u : (E < LOG_NEAR1_E1 ? 0xFFFFFFFFu : LOG_NEAR1_HI);
  f.pad = 0;
  return f;
}
struct Log10ArgFold {
  uint32_t hx, lo; // as in Log10Arg
  int xoff;        // ky << 4: the byte offset of ky's pair from the pair of ky = 0
};
// the two exponent fields of the select, for a kernel that holds them in vector registers (pin_fold_constants): as operands
// of a v_cndmask_b32 they must be there, and left to itself the compiler copies them anew for every logarithm
struct FoldPins {
  uint32_t below, above; // 0x3FE00000, 0x3FF00000
};
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ FoldPins pin_fold_constants() {
  FoldPins p;
  asm volatile("v_mov_b32 %0, %1" : "=v"(p.below) : "s"(0x3FE00000u));
  asm volatile("v_mov_b32 %0, %1" : "=v"(p.above) : "s"(0x3FF00000u));
  return p;
}
// one compare and one v_cndmask_b32, nothing else
__device__ __forceinline__ uint32_t fold_exponent_field(uint32_t hi, const FoldPins &p) {
  uint32_t sel;
  asm("v_cmp_gt_u32 vcc, %3, %1\n\tv_cndmask_b32 %0, %3, %2, vcc" : "=v"(sel) : "v"(hi), "v"(p.below), "v"(p.above) : "vcc");
  return sel;
}
#else
inline FoldPins pin_fold_constants() { return FoldPins{0x3FE00000u, 0x3FF00000u}; }
inline uint32_t fold_exponent_field(uint32_t hi, const FoldPins &p) { return hi < p.above ? p.below : p.above; }
#endif
C2R_MHD Log10ArgFold log10_split_fold(double x, const FoldPins *fp = nullptr) { // x positive, normal, finite
  const uint64_t ix = asuint64(x);
  const uint32_t hi = (uint32_t)(ix >> 32);
  Log10ArgFold a;
  a.lo = (uint32_t)ix;
  const uint32_t field = fp ? fold_exponent_field(hi, *fp) : (hi < 0x3FF00000u ? 0x3FE00000u : 0x3FF00000u);
  a.hx = (hi & 0x000FFFFFu) | field;
  a.xoff = (int)(hi - a.hx) >> 16;
  return a;
}
C2R_MHD bool log10_near1(const Log10ArgFold &a) { return a.hx - 0x3FEE0000u < 0x00030900u; }
// the same test by the limit of hx's own table entry (LogFold::lim)
C2R_MHD bool log10_near1(const Log10ArgFold &a, uint32_t lim) { return a.hx < lim; }
C2R_MHD double log10_arg_value(const Log10ArgFold &a) { return asdouble(((uint64_t)a.hx << 32) | a.lo); }
// log_table_path4 with z = x' and no kshift; `lim`, where given, receives the entry's near-1 limit, read in one piece with c
C2R_MHD double log_table_path_fold(const Log10ArgFold &a, const LogFold *tab, const LogPins *pins = nullptr, uint32_t *lim = nullptr) {
  const double *A = GMT(log_hdr) + 2;
  const double A1 = pins ? pins->a1 : A[1], A3 = pins ? pins->a3 : A[3];
  const uint32_t T = a.hx - 0x3FE00000u;  // [0, 0x200000)
  const uint32_t off = (T >> 8) & 0x1FE0u; // entry T >> 13 of 32-byte entries
  const LogFold *e = (const LogFold *)((const char *)tab + off);
  const double invc = e->invc, w = e->w;
#if defined(__HIP_DEVICE_COMPILE__)
  // c and the limit as the one 16-byte piece they are (two reads per entry, as without the limit)
  typedef uint32_t LogFoldTail __attribute__((ext_vector_type(4)));
  const LogFoldTail t = *(const LogFoldTail *)&e->c;
  const double c = asdouble(((uint64_t)t.y << 32) | t.x);
  if (lim) *lim = t.z;
#else
  const double c = e->c;
  if (lim) *lim = e->lim;
#endif
  const double r = fma_(log10_arg_value(a), invc, -1.0);
  const double t1 = fma_kc(r, A[2], A1);
  const double hi_ = r + w;
  const double r2 = r * r;
  double lo_ = (w - hi_) + r;
  lo_ = lo_ + c;
  const double r3 = r * r2;
  const double t2 = fma_kc(r, A[4], A3);
  const double s_ = fma_(r2, A[0], lo_);
  const double p_ = fma_(t2, r2, t1);
  const double q_ = fma_(r3, p_, s_);
  return q_ + hi_;
}
// `x0`: the pair of ky = 0, entry -LOG10_KY_LO of a table filled like Log10Exp's; precondition as there
C2R_MHD double log10_finish(const Log10ArgFold &a, double lg, const Log10Exp *x0) {
  const double ivln10 = asdouble(0x3FDBCB7B1526E50EULL);
  const Log10Exp *e = (const Log10Exp *)((const char *)x0 + a.xoff);
  const double ylo = e->ylo, yhi = e->yhi;
  const double zz = ylo + ivln10 * lg;
  return zz + yhi;
}
// the folded table, the exponent table from its ky = 0 entry, and the select's two constants: a type of its own again
struct LogFoldExp {
  const LogFold *tab;
  const Log10Exp *exp0;
  const FoldPins *fold;
};
// log10_norm: the caller guarantees a positive, normal, finite argument (tau_table_position passes
// max(1e-20, tau)); log10_pos adds the check and falls back to log10_.
C2R_MHD double log10_norm(double x, const double *tab) {
  const Log10Arg a = log10_split(x);
  const double lg = log10_near1(a) ? log_near1(log10_arg_value(a)) : log_table_path(a, tab);
  return log10_finish(a, lg);
}
C2R_MHD const double *log_table() { return GMT(log_tab); }
C2R_MHD double log10_norm(double x) { return log10_norm(x, GMT(log_tab)); }
// the same with the (invc, logc) table wherever the caller keeps it (LDS)
C2R_MHD double log10_pos(double x, const double *tab) {
  const uint32_t hi = (uint32_t)(asuint64(x) >> 32);
  if (hi - 0x00100000u >= 0x7FE00000u) return log10_(x); // zero, subnormal, negative, inf, nan
  return log10_norm(x, tab);
}
C2R_MHD double log10_pos(double x) {
  const uint32_t hi = (uint32_t)(asuint64(x) >> 32);
  if (hi - 0x00100000u >= 0x7FE00000u) return log10_(x); // zero, subnormal, negative, inf, nan
  return log10_norm(x);
}

// ---- exp: __exp_fma ----------------------------------------------------------------------------
C2R_MHD double exp_special(double tmp, uint64_t sbits, uint64_t ki) {
  if ((ki & 0x80000000ULL) == 0) { // k > 0: the exponent of scale might have overflowed
    sbits -= 1009ULL << 52;
    const double scale = asdouble(sbits);
    return 0x1p1009 * fma_(scale, tmp, scale);
  }
  sbits += 1022ULL << 52; // k < 0: careful in the subnormal range
  const double scale = asdouble(sbits);
  const double st = scale * tmp;
  double y = scale + st;
  if (y < 1.0) {
    const double hi = 1.0 + y;
    const double lo = (scale - y) + st;
    double t = 1.0 - hi;
    t = t + y;
    t = t + lo;
    y = (t + hi) - 1.0;
    if (y == 0.0) y = 0.0;
  }
  return 0x1p-1022 * y;
}

// shared tail of exp and pow's exp_inline: r already reduced, ki = bits of the shifted k
C2R_MHD double exp_poly(double r, uint64_t ki, uint32_t abstop) {
  const double *H = GMT(exp_hdr);
  const double C2 = H[4], C3 = H[5], C4 = H[6], C5 = H[7];
  const int idx = 2 * (int)(ki & 127);
  const uint64_t top = ki << 45;
  const double tail = asdouble(GMT(exp_tab)[idx]);
  const uint64_t sbits = GMT(exp_tab)[idx + 1] + top;
  const double a = fma_(r, C3, C2);
  const double b = r + tail;
  const double r2 = r * r;
  const double c = fma_(r, C5, C4);
  const double d = fma_(a, r2, b);
  const double r4 = r2 * r2;
  const double tmp = fma_(r4, c, d);
  if (abstop == 0) return exp_special(tmp, sbits, ki);
  const double scale = asdouble(sbits);
  return fma_(scale, tmp, scale);
}

C2R_MHD double exp_(double x) {
  const double *H = GMT(exp_hdr);
  const double InvLn2N = H[0], Shift = H[1], NegLn2hiN = H[2], NegLn2loN = H[3];
  uint32_t abstop = (uint32_t)(asuint64(x) >> 52) & 0x7ff;
  if (abstop - 0x3c9u > 0x3eu) {
    if ((int32_t)(abstop - 0x3c9u) < 0) return 1.0 + x; // |x| < 2^-54
    if (abstop >= 0x409u) {                            // |x| >= 1024, inf, nan
      if (asuint64(x) == 0xFFF0000000000000ULL) return 0.0;
      if (abstop >= 0x7ffu) return 1.0 + x;
      return (asuint64(x) >> 63) ? 0.0 : (double)INFINITY;
    }
    abstop = 0; // 512 <= |x| < 1024: handled by exp_special
  }
  const double kds = fma_(x, InvLn2N, Shift);
  const uint64_t ki = asuint64(kds);
  const double kd = kds - Shift;
  double r = fma_(kd, NegLn2hiN, x);
  r = fma_(kd, NegLn2loN, r);
  return exp_poly(r, ki, abstop);
}

// ---- pow: __pow_fma ----------------------------------------------------------------------------
// x <= 0, subnormal, inf, nan, or |y| < 2^-65 / >= 2^63: never reached on the hot path (bases are
// temperatures, ratios of temperatures and ionised fractions >= 1e-20; exponents are fit constants).
// Kept out of line so that the platform pow's code and registers stay out of the kernels.
#if defined(__HIPCC__)
__host__ __device__ __attribute__((noinline)) inline double pow_out_of_domain(double x, double y) { return ::pow(x, y); }
#else
inline double pow_out_of_domain(double x, double y) { return ::pow(x, y); }
#endif

C2R_MHD double pow_(double x, double y) {
  const uint64_t ix = asuint64(x), iy = asuint64(y);
  const uint32_t topx = (uint32_t)(ix >> 52), topy = (uint32_t)(iy >> 52);
  if (topx - 1u > 0x7fdu || (topy & 0x7ffu) - 0x3beu > 0x7fu) return pow_out_of_domain(x, y);
  // log_inline
  const double *H = GMT(pow_hdr);
  const double Ln2hi = H[0], Ln2lo = H[1];
  const double *A = H + 2;
  const uint64_t tmp = ix - 0x3FE6955500000000ULL; // OFF
  const int i = (int)((tmp >> 45) & 127);
  const int k = (int)((int64_t)tmp >> 52);
  const uint64_t iz = ix - (tmp & 0xFFF0000000000000ULL);
  const double z = asdouble(iz);
  const double kd = (double)k;
  const double invc = GMT(pow_tab)[3 * i], logc = GMT(pow_tab)[3 * i + 1], logctail = GMT(pow_tab)[3 * i + 2];
  const double t1 = fma_(kd, Ln2hi, logc);
  const double r = fma_(z, invc, -1.0);
  const double ar = r * A[0];
  const double lo1 = fma_(kd, Ln2lo, logctail);
  const double q1 = fma_(r, A[2], A[1]);
  const double q2 = fma_(r, A[4], A[3]);
  const double t2 = r + t1;
  const double ar2 = r * ar;
  const double ar3 = r * ar2;
  const double lo3 = fma_(ar, r, -ar2);
  const double lo2 = (t1 - t2) + r;
  const double q3 = fma_(r, A[6], A[5]);
  const double hi = t2 + ar2;
  const double q4 = fma_(q3, ar2, q2);
  const double lo4 = (t2 - hi) + ar2;
  const double q5 = fma_(ar2, q4, q1);
  double lo = lo1 + lo2;
  lo = lo + lo3;
  lo = lo + lo4;
  lo = fma_(ar3, q5, lo);
  const double lhi = hi + lo;
  const double ltail = (hi - lhi) + lo;
  const double ehi = y * lhi;
  const double elo = fma_(y, ltail, fma_(lhi, y, -ehi));
  // exp_inline(ehi, elo, sign_bias = 0)
  const double *E = GMT(exp_hdr);
  const double InvLn2N = E[0], Shift = E[1], NegLn2hiN = E[2], NegLn2loN = E[3];
  uint32_t abstop = (uint32_t)(asuint64(ehi) >> 52) & 0x7ff;
  if (abstop - 0x3c9u > 0x3eu) {
    if ((int32_t)(abstop - 0x3c9u) < 0) return 1.0 + ehi;
    if (abstop >= 0x409u) return (asuint64(ehi) >> 63) ? 0.0 : (double)INFINITY;
    abstop = 0;
  }
  const double kds = fma_(ehi, InvLn2N, Shift);
  const uint64_t ki = asuint64(kds);
  const double kd2 = kds - Shift;
  double rr = fma_(kd2, NegLn2hiN, ehi);
  rr = fma_(kd2, NegLn2loN, rr);
  rr = elo + rr;
  return exp_poly(rr, ki, abstop);
}

#undef GMT
} // namespace gm
} // namespace c2r

// route the physics through these (c2ray_device.hpp checks for C2R_MATH_EXP)
#define C2R_MATH_EXP(x) ::c2r::gm::exp_(x)
#define C2R_MATH_LOG10(x) ::c2r::gm::log10_(x)
#define C2R_MATH_LOG10P(x) ::c2r::gm::log10_pos(x)
#define C2R_MATH_LOG10PT(x, tab) ::c2r::gm::log10_pos(x, tab)
#define C2R_MATH_LOG10N(x) ::c2r::gm::log10_norm(x)
#define C2R_MATH_POW(x, y) ::c2r::gm::pow_(x, y)
