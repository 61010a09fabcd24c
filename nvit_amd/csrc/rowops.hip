// Row-wise fp32 kernels on the residual stream: normalised LERP (+norm_skip) forward/backward,
// per-head cosine normalisation forward/backward, SwiGLU gate forward/backward, and the small
// column reductions that turn per-block partial sums into parameter gradients.
// HBM-bound: one wave owns one row (16-byte loads, all reductions by lane shuffles), rows are
// grid-strided, per-column partial sums stay in registers until the wave's last row.
#include "dispatch.h"

namespace {

constexpr int ROW_WAVES = NVIT_ROW_WAVES;  // waves (rows in flight) per 256-thread workgroup
static_assert(ROW_WAVES * 64 == 256, "the row kernels launch 256 threads");

// Each lane owns NV float4 groups of a row: columns (i*64 + lane)*4 .. +3, i < NV, while < C.
template <int NV>
struct RowVec {
  f32x4 v[NV];
};

template <int NV, typename T>
__device__ __forceinline__ void row_load(RowVec<NV>& r, const T* p, int C, int lane) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    r.v[i] = c < C ? load4<T>(p + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}
template <int NV, typename T>
__device__ __forceinline__ void row_store(const RowVec<NV>& r, T* p, int C, int lane) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < C) store4<T>(p + c, r.v[i]);
  }
}
template <int NV>
__device__ __forceinline__ float row_dot(const RowVec<NV>& a, const RowVec<NV>& b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += a.v[i][0] * b.v[i][0] + a.v[i][1] * b.v[i][1] + a.v[i][2] * b.v[i][2] + a.v[i][3] * b.v[i][3];
  return wave_sum(s);
}

// Streaming (non-temporal) loads of read-once fp32 rows: the residual stream and the incoming gradient are not read again
// soon, keeping them out of the caches leaves room for what the neighbouring GEMMs re-read (measured on the whole step:
// backward -0.34 ms in round 3, forward -0.35 ms in round 4; streaming STORES of the backward outputs: +-0, not used).
template <int NV>
__device__ __forceinline__ void row_load_f32_nt(RowVec<NV>& r, const float* p, int C, int lane) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    r.v[i] = c < C ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + c)) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}

// ------------------------------------------------------------------------------ LERP forward
struct LerpFwdArgs {
  const float* h;
  const void* y;
  const float* alpha;
  float c_a;
  const float* skip_x;
  const float* skip;
  float* out;
  void* out_lo;
  int M, C;
  const float* gate;   // GATED kernels: one fp32 gate per sample (DropPath), rows m*T .. m*T+T-1 belong to sample m
  int T;
};

// The gate of row m's sample.  A wave owns one row, so m is the same in all its lanes: the index is taken from the first
// lane and the table read through the constant address space (nothing writes it while a row kernel runs) - one scalar
// load per row, no vector register.
__device__ __forceinline__ float row_gate(const float* gate, int m, int T) {
  typedef const __attribute__((address_space(4))) float* cfloat_p;
  return ((cfloat_p)gate)[__builtin_amdgcn_readfirstlane(m) / T];
}

// GATED (stochastic depth): the row's step sizes are gate * |alpha*c_a|, so a dropped sample (gate 0) leaves nrm(h).  A
// template switch like those of lerp_bwd_kernel; with gate 1.0f the products are exact and the bits those of the plain
// kernel.
template <int NV, typename TY, typename TL, bool GATED>
__global__ __launch_bounds__(256) void lerp_fwd_kernel(LerpFwdArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  RowVec<NV> lam;
  row_load<NV, float>(lam, a.alpha, a.C, lane);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) lam.v[i][e] = fabsf(lam.v[i][e] * a.c_a);
  const float skip = a.skip_x ? a.skip[0] : 0.f;
  for (int m = blockIdx.x * ROW_WAVES + wid; m < a.M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> x, y, r, xs;
    row_load_f32_nt<NV>(x, a.h + (size_t)m * a.C, a.C, lane);   // (the residual stream is read once here: streaming load)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if constexpr (sizeof(TY) == 2) {
        uint2 raw = make_uint2(0u, 0u);
        if (c < a.C) {
          typedef unsigned int u32x2_ __attribute__((ext_vector_type(2)));
          raw = __builtin_bit_cast(uint2, __builtin_nontemporal_load(reinterpret_cast<const u32x2_*>(reinterpret_cast<const TY*>(a.y) + (size_t)m * a.C + c)));
        }
        const bf16x4 b4 = __builtin_bit_cast(bf16x4, raw);
        y.v[i] = (f32x4){(float)b4[0], (float)b4[1], (float)b4[2], (float)b4[3]};
      } else {
        y.v[i] = c < a.C ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.y) + (size_t)m * a.C + c)) : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    if (a.skip_x) row_load_f32_nt<NV>(xs, a.skip_x + (size_t)m * a.C, a.C, lane);   // with the others: one round trip per row
    float gt = 1.0f;
    if constexpr (GATED) gt = row_gate(a.gate, m, a.T);
    const float rsx = 1.0f / sqrtf(row_dot<NV>(x, x));
    const float rsy = 1.0f / sqrtf(row_dot<NV>(y, y));
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const f32x4 av = x.v[i] * rsx, bv = y.v[i] * rsy;
      if constexpr (GATED) r.v[i] = av + (lam.v[i] * gt) * (bv - av);
      else r.v[i] = av + lam.v[i] * (bv - av);
    }
    const float rsr = 1.0f / sqrtf(row_dot<NV>(r, r));
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = r.v[i] * rsr;
    if (a.skip_x) {
#pragma unroll
      for (int i = 0; i < NV; ++i) r.v[i] = r.v[i] * skip + xs.v[i];
      const float rst = 1.0f / sqrtf(row_dot<NV>(r, r));
#pragma unroll
      for (int i = 0; i < NV; ++i) r.v[i] = r.v[i] * rst;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {   // the fp32 stream is read again only far later (next block / backward): streaming store
      const int c = (i * 64 + lane) * 4;
      if (c < a.C) __builtin_nontemporal_store(r.v[i], reinterpret_cast<f32x4*>(a.out + (size_t)m * a.C + c));
    }
    if (a.out_lo) row_store<NV, TL>(r, reinterpret_cast<TL*>(a.out_lo) + (size_t)m * a.C, a.C, lane);
  }
}

// ------------------------------------------------------------------------------ LERP backward
struct LerpBwdArgs {
  const float* dout;
  const bf16* dout_add;   // optional second addend of the incoming gradient (a data-gradient GEMM's bf16 output), or NULL
  const float* h;
  const void* y;
  const float* alpha;
  float c_a;
  const float* skip_x;
  const float* skip;
  float* dh;
  int accum_dh;
  float* dy;
  void* dy_lo;
  float* dskip_x;
  float* part_dlam;
  float* part_dskip;
  int M, C;
  const float* gate;   // GATED kernels: as in LerpFwdArgs
  int T;
};

// ADD: the incoming gradient has a second, bf16 addend (a.dout_add).  A template switch, not a run-time test: with the test
// inside the row loop hipcc waits for the addend right where it is loaded, before the remaining loads of the row have
// been issued - a second memory round trip per row (+137 us per Base block, measured).
//
// Register-lean form: per row only the two unit vectors a, b and the running gradient g stay in registers (plus the
// per-column step sizes and their gradient sums); the LERP output o = (a + lam*(b - a)) * rsr is recomputed where it is
// needed (three flops per element) and da / db are formed at the store.  No LDS: every wave writes its own row of
// column partials (part_dlam [4*nblk, C], part_dskip [4*nblk]).  At C = 768 this is 104 registers instead of 160
// (4 waves per SIMD instead of 3) - small enough to be co-resident with two waves of the 193-register weight-gradient
// GEMM on the same SIMD.
template <int NV>
__device__ __forceinline__ float dot4(const f32x4& a, const f32x4& b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
}

// SKIP (norm_skip fused behind the LERP: the MLP half of a block) and ACCUM (dh += : the attention half, whose dh already
// holds the gradient of the skip path) are template switches as well: a row then keeps 5 vectors in flight instead of 6.
// GATED (stochastic depth, see lerp_fwd_kernel): the row's step sizes are gate * lam wherever lam is used, and the row's
// term of d(lam) carries the gate; the gate sits in a scalar register and the products are formed where they are used.
template <int NV, typename TY, typename TL, bool ADD, bool SKIP, bool ACCUM, bool GATED>
__global__ __launch_bounds__(256, 1) void lerp_bwd_kernel(LerpBwdArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  RowVec<NV> lam, dlam;
  row_load<NV, float>(lam, a.alpha, a.C, lane);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    dlam.v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) lam.v[i][e] = fabsf(lam.v[i][e] * a.c_a);
  }
  const float skip = SKIP ? a.skip[0] : 0.f;
  float dskip_acc = 0.f;
  for (int m = blockIdx.x * ROW_WAVES + wid; m < a.M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> av, bv, g, t, old;   // av: h then a = nrm(h); bv: y then b = nrm(y); g: incoming gradient, then d(lerp out), then dr
    uint2 ga[NV];                    // the bf16 addend stays packed until it is added (half the registers in flight)
    const size_t ro = (size_t)m * a.C;
    // every load of the row goes out before the first reduction: one memory round trip per row, not two or three
    row_load_f32_nt<NV>(av, a.h + ro, a.C, lane);
    row_load<NV, TY>(bv, reinterpret_cast<const TY*>(a.y) + ro, a.C, lane);
    row_load_f32_nt<NV>(g, a.dout + ro, a.C, lane);
    if constexpr (ADD) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        ga[i] = c < a.C ? *reinterpret_cast<const uint2*>(a.dout_add + ro + c) : make_uint2(0u, 0u);
      }
    }
    if constexpr (SKIP) row_load_f32_nt<NV>(t, a.skip_x + ro, a.C, lane);
    float gt = 1.0f;
    if constexpr (GATED) gt = row_gate(a.gate, m, a.T);
#define NVIT_LAM(i_) (GATED ? lam.v[i_] * gt : lam.v[i_])   /* the row's step sizes */
    if constexpr (ADD) {   // incoming gradient = dout + dout_add: the GEMM that produced dout_add need not read-modify-write dout
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const bf16x4 q = __builtin_bit_cast(bf16x4, ga[i]);
        g.v[i] += (f32x4){(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
      }
    }
    const float rsx = 1.0f / sqrtf(row_dot<NV>(av, av));
    const float rsy = 1.0f / sqrtf(row_dot<NV>(bv, bv));
    // (the old dh values are needed only at the store: requested here, they arrive under the remaining reductions)
    if constexpr (ACCUM) row_load<NV, float>(old, a.dh + ro, a.C, lane);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      av.v[i] = av.v[i] * rsx;
      bv.v[i] = bv.v[i] * rsy;
      const f32x4 ou = av.v[i] + NVIT_LAM(i) * (bv.v[i] - av.v[i]);
      ss += dot4<NV>(ou, ou);
    }
    const float rsr = 1.0f / sqrtf(wave_sum(ss));
#define NVIT_LERP_O(i_) ((av.v[i_] + NVIT_LAM(i_) * (bv.v[i_] - av.v[i_])) * rsr)   /* o = lerp output (unit norm), recomputed */
    if constexpr (SKIP) {
      // t = o*skip + xs ; out = t/|t| ; dt = (g - out<out,g>)/|t| ; do = skip*dt ; dxs = dt ; dskip += <dt,o>
      float st = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        t.v[i] = NVIT_LERP_O(i) * skip + t.v[i];
        st += dot4<NV>(t.v[i], t.v[i]);
      }
      const float rst = 1.0f / sqrtf(wave_sum(st));
      float tg = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        t.v[i] = t.v[i] * rst;
        tg += dot4<NV>(t.v[i], g.v[i]);
      }
      tg = wave_sum(tg);
      float dso = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        g.v[i] = (g.v[i] - t.v[i] * tg) * rst;   // g = dt
        dso += dot4<NV>(g.v[i], NVIT_LERP_O(i));
      }
      row_store<NV, float>(g, a.dskip_x + ro, a.C, lane);
      dskip_acc += wave_sum(dso);
#pragma unroll
      for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] * skip;   // g = d(lerp output)
    }
    // dr = (g - o<o,g>) * rsr
    float og = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) og += dot4<NV>(NVIT_LERP_O(i), g.v[i]);
    og = wave_sum(og);
    float ada = 0.f, bdb = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      g.v[i] = (g.v[i] - NVIT_LERP_O(i) * og) * rsr;   // g = dr
      dlam.v[i] += (GATED ? g.v[i] * gt : g.v[i]) * (bv.v[i] - av.v[i]);
      const f32x4 db = NVIT_LAM(i) * g.v[i];
      ada += dot4<NV>(av.v[i], g.v[i] - db);
      bdb += dot4<NV>(bv.v[i], db);
    }
#undef NVIT_LERP_O
    ada = wave_sum(ada);
    bdb = wave_sum(bdb);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const f32x4 db = NVIT_LAM(i) * g.v[i];
      f32x4 dh = ((g.v[i] - db) - av.v[i] * ada) * rsx;
      const f32x4 dy = (db - bv.v[i] * bdb) * rsy;
      if constexpr (ACCUM) dh += old.v[i];
      if (c < a.C) {
        store4<float>(a.dh + ro + c, dh);
        if (a.dy) store4<float>(a.dy + ro + c, dy);
        if (a.dy_lo) store4<TL>(reinterpret_cast<TL*>(a.dy_lo) + ro + c, dy);
      }
    }
#undef NVIT_LAM
  }
  // column partials: one row per wave (fixed layout, reduced in fixed order by nvit_colsum_reduce)
  const size_t prow = (size_t)blockIdx.x * ROW_WAVES + wid;
  row_store<NV, float>(dlam, a.part_dlam + prow * a.C, a.C, lane);
  if (SKIP && lane == 0) a.part_dskip[prow] = dskip_acc;
}

// ------------------------------------------------------------------------------ standalone norm_skip
// out = nrm(source*skip + target)  (Block.norm_skip, reference model.py:84-87) for callers that use it on its own;
// ViT.forward uses the version fused into lerp_fwd/bwd.
template <int NV>
__global__ __launch_bounds__(256) void norm_skip_fwd_kernel(const float* src, const float* tgt, const float* skip,
                                                             float* out, int M, int C) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float sk = skip[0];
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> a, b;
    row_load<NV, float>(a, src + (size_t)m * C, C, lane);
    if (tgt) {   // tgt == NULL: plain justnorm(source * skip)
      row_load<NV, float>(b, tgt + (size_t)m * C, C, lane);
#pragma unroll
      for (int i = 0; i < NV; ++i) a.v[i] = a.v[i] * sk + b.v[i];
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) a.v[i] = a.v[i] * sk;
    }
    const float rs = 1.0f / sqrtf(row_dot<NV>(a, a));
#pragma unroll
    for (int i = 0; i < NV; ++i) a.v[i] = a.v[i] * rs;
    row_store<NV, float>(a, out + (size_t)m * C, C, lane);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void norm_skip_bwd_kernel(const float* dout, const float* src, const float* tgt,
                                                             const float* skip, float* dsrc, float* dtgt,
                                                             float* part_dskip, int M, int C) {
  __shared__ float red[ROW_WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float sk = skip[0];
  float acc = 0.f;
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> a, b, g;
    row_load<NV, float>(a, src + (size_t)m * C, C, lane);
    if (tgt) {
      row_load<NV, float>(b, tgt + (size_t)m * C, C, lane);
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) b.v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    row_load<NV, float>(g, dout + (size_t)m * C, C, lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) b.v[i] = a.v[i] * sk + b.v[i];
    const float rs = 1.0f / sqrtf(row_dot<NV>(b, b));
#pragma unroll
    for (int i = 0; i < NV; ++i) b.v[i] = b.v[i] * rs;
    const float og = row_dot<NV>(b, g);
#pragma unroll
    for (int i = 0; i < NV; ++i) g.v[i] = (g.v[i] - b.v[i] * og) * rs;  // d(source*skip + target)
    acc += row_dot<NV>(g, a);
    if (dtgt) row_store<NV, float>(g, dtgt + (size_t)m * C, C, lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] * sk;
    row_store<NV, float>(g, dsrc + (size_t)m * C, C, lane);
  }
  if (lane == 0) red[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part_dskip[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------ head split / merge (+ q/k normalise)
// Compact heads (d = 16, 32, 64, 128) are stored d wide.  Head dims d < 128 that are no power of two (72, 80, 88, 104) run
// on the D = 128 attention kernels: their head tensors are [B,H,T,PAD_D] with columns d..PAD_D-1 stored as zeros, which
// change no score, no output column < d and no gradient column < d.  DP is the stored head width, d <= DP the real one.
// heads_pad_fwd_kernel and heads_merge_kernel index a row in STORED coordinates: lane l of pass p owns columns pc..pc+3 of
// the H*DP wide stored row, pc = p*256 + 4l, so a head is always one aligned group of DP/4 lanes whatever d is, and the
// lanes with pc % DP >= d load nothing and store the zeros.  With d == DP every lane inside the row is live and the stored
// column is the token-major one: heads_merge_kernel is the backward of both layouts.  The forward keeps a kernel per
// layout: the compact one issues all of a row's loads before any arithmetic, which the pass loop lost to at d = 128.
constexpr int PAD_D = NVIT_PAD_HEAD_DIM;

struct QkArgs {
  const void *q, *k, *v;   // projection outputs, token-major with row strides ld*
  int ldq, ldk, ldv;
  const float* sqk;
  float c_q;
  void *qh, *kh, *vh;
  float *rq, *rk;
  float* sqk_pad;   // padded heads only: [H*PAD_D], sqk with zero pads, for nvit_attn_fwd_bounded at D = PAD_D (NORM; may be NULL)
  int B, T, H, d;
};

// A lane's four terms of a head's dot product, in two roundings: one fma chain, or every product rounded before the
// sum.  Which dot product takes which is part of every output's bits (profiles/heads_unify_bitwise.log) and differs
// between the layouts: sq sums and dk_ chains everywhere, sk chains on compact heads and sums on padded ones, dq_ the
// other way round.  The order of the chain is load-bearing too - term 1 first, then 0, 2, 3 - do not tidy it.  Giving
// both layouts one rounding is a numerical change of its own.
__device__ __forceinline__ float dot4_fma(f32x4 a, f32x4 b) {
  return __builtin_fmaf(a[3], b[3], __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[0], b[0], a[1] * b[1])));
}
__device__ __forceinline__ float dot4_sum(f32x4 a, f32x4 b) {
#pragma clang fp contract(off)
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
}

// qknorm_fwd_kernel: qh/kh/vh [B,H,T,d] (compact) from token-major q/k/v; the row sits in NV register vectors.  NORM: q and
// k normalised per head from the unrounded projections and scaled by sqk*c_q, one rounding at the head tensors, rq / rk
// [M,H] = the inverse norms.  NORM = false (sqk == NULL): the head split alone, q and k copied as they are (the plain-ViT
// attention, reference model.py:97-100 without :104-112); rq / rk are not written.
template <int NV, typename TI, typename T, bool NORM>   // TI: type of the projection outputs read, T: type of the head tensors written
__global__ __launch_bounds__(256) void qknorm_fwd_kernel(QkArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int C = a.H * a.d, M = a.B * a.T, G = a.d >> 2;  // lanes per head
  RowVec<NV> s;
  if constexpr (NORM) {
    row_load<NV, float>(s, a.sqk, C, lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) s.v[i] = s.v[i] * a.c_q;
  }
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    const int b = m / a.T, t = m % a.T;
    RowVec<NV> q, k, v;
    row_load<NV, TI>(q, reinterpret_cast<const TI*>(a.q) + (size_t)m * a.ldq, C, lane);
    row_load<NV, TI>(k, reinterpret_cast<const TI*>(a.k) + (size_t)m * a.ldk, C, lane);
    row_load<NV, TI>(v, reinterpret_cast<const TI*>(a.v) + (size_t)m * a.ldv, C, lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const int h = c / a.d, j = c % a.d;
      const size_t dst = (((size_t)b * a.H + h) * a.T + t) * a.d + j;
      if constexpr (!NORM) {
        if (c < C) {
          store4<T>(reinterpret_cast<T*>(a.qh) + dst, q.v[i]);
          store4<T>(reinterpret_cast<T*>(a.kh) + dst, k.v[i]);
          store4<T>(reinterpret_cast<T*>(a.vh) + dst, v.v[i]);
        }
      } else {
        const float sq = group_sum_dyn(dot4_sum(q.v[i], q.v[i]), G), sk = group_sum_dyn(dot4_fma(k.v[i], k.v[i]), G);
        if (c < C) {
          const float rq = 1.0f / sqrtf(sq), rk = 1.0f / sqrtf(sk);
          store4<T>(reinterpret_cast<T*>(a.qh) + dst, q.v[i] * rq * s.v[i]);
          store4<T>(reinterpret_cast<T*>(a.kh) + dst, k.v[i] * rk * s.v[i]);
          store4<T>(reinterpret_cast<T*>(a.vh) + dst, v.v[i]);
          if (j == 0) {
            a.rq[(size_t)m * a.H + h] = rq;
            a.rk[(size_t)m * a.H + h] = rk;
          }
        }
      }
    }
  }
}

// heads_pad_fwd_kernel: qknorm_fwd_kernel from fp32 projections into zero-padded head tensors [B,H,T,PAD_D].  Every launch
// stores every pad column.
template <typename T, bool NORM>
__global__ __launch_bounds__(256) void heads_pad_fwd_kernel(QkArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int M = a.B * a.T, HP = a.H * PAD_D;
  const float *aq = reinterpret_cast<const float*>(a.q), *ak = reinterpret_cast<const float*>(a.k),
              *av = reinterpret_cast<const float*>(a.v);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if constexpr (NORM) {
    if (a.sqk_pad && blockIdx.x == 0) {
      for (int pc = threadIdx.x * 4; pc < HP; pc += 1024) {
        const int h = pc / PAD_D, j = pc % PAD_D;
        store4<float>(a.sqk_pad + pc, j < a.d ? load4<float>(a.sqk + h * a.d + j) : z);
      }
    }
  }
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    const int b = m / a.T, t = m % a.T;
    for (int p0 = 0; p0 < HP; p0 += 256) {
      const int pc = p0 + lane * 4;
      const int h = pc / PAD_D, j = pc % PAD_D;
      const bool in = pc < HP, live = in && j < a.d;
      const int c = h * a.d + j;
      f32x4 q = live ? load4<float>(aq + (size_t)m * a.ldq + c) : z;
      f32x4 k = live ? load4<float>(ak + (size_t)m * a.ldk + c) : z;
      const f32x4 v = live ? load4<float>(av + (size_t)m * a.ldv + c) : z;
      if constexpr (NORM) {
        const f32x4 s = live ? load4<float>(a.sqk + c) * a.c_q : z;
        const float sq = group_sum<32>(dot4_sum(q, q)), sk = group_sum<32>(dot4_sum(k, k));
        const float rq = 1.0f / sqrtf(sq), rk = 1.0f / sqrtf(sk);
        q = live ? q * rq * s : z;   // (the pads are zeros even where a head's norm is 0 or not finite)
        k = live ? k * rk * s : z;
        if (in && j == 0) {
          a.rq[(size_t)m * a.H + h] = rq;
          a.rk[(size_t)m * a.H + h] = rk;
        }
      }
      if (in) {
        const size_t dst = (((size_t)b * a.H + h) * a.T + t) * PAD_D + j;
        store4<T>(reinterpret_cast<T*>(a.qh) + dst, q);
        store4<T>(reinterpret_cast<T*>(a.kh) + dst, k);
        store4<T>(reinterpret_cast<T*>(a.vh) + dst, v);
      }
    }
  }
}

struct QkBwdArgs {
  const void *dqh, *dkh, *dvh, *qh, *kh;
  const float *rq, *rk, *sqk;
  float c_q;
  void *dq, *dk, *dv;
  int ldq, ldk, ldv;
  float* part;
  int B, T, H, d;
};

// heads_merge_kernel: the backward of both forward kernels: dq/dk/dv (type T, row strides ld*) from the first d columns of
// every head of dqh/dkh/dvh [B,H,T,DP] (pad columns are never read).  NORM = false: the head merge alone, two passes
// of a row per loop iteration; NORM: one pass per iteration, through
// the normalise as well, and part [gridDim.x, C] = each workgroup's d(sqk*c_q).  Dynamic LDS with NORM, (ROW_WAVES + 2) * C
// floats (at most 48 KiB), none without: a wave accumulates its partials in its own row of C floats, and s = sqk*c_q and
// 1/s are computed once per workgroup into two more, all in token-major channel order.
template <int DP, typename T, bool NORM>
__global__ __launch_bounds__(256) void heads_merge_kernel(QkBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float merge_red[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int C = a.H * a.d, M = a.B * a.T, HP = a.H * DP;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  float* red = merge_red + wid * C;
  const float *s_row = merge_red + ROW_WAVES * C, *sinv_row = s_row + C;
  if constexpr (NORM) {
    for (int c = threadIdx.x; c < ROW_WAVES * C; c += 256) merge_red[c] = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
      const float s = a.sqk[c] * a.c_q;
      merge_red[ROW_WAVES * C + c] = s;
      merge_red[(ROW_WAVES + 1) * C + c] = s != 0.f ? 1.0f / s : 0.f;
    }
    __syncthreads();
  }
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    const int b = m / a.T, t = m % a.T;
    if constexpr (!NORM) {
      // The merge alone: the loads of two passes go out before the first store.  Loads and stores share one in-order
      // counter, so a load behind a store waits for that store's acknowledgement too; one pass per iteration lost 6 % to
      // the compile-time unrolled kernel this one replaced at d = 64 (profiles/heads_unify_ab.log).
      for (int p0 = 0; p0 < HP; p0 += 512) {
        f32x4 g[2][3];
        int c[2];
        bool live[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int pc = p0 + u * 256 + lane * 4;
          const int h = pc / DP, j = pc % DP;
          live[u] = pc < HP && j < a.d;
          c[u] = h * a.d + j;
          const size_t src = (((size_t)b * a.H + h) * a.T + t) * DP + j;
          g[u][0] = live[u] ? load4<T>(reinterpret_cast<const T*>(a.dqh) + src) : z;
          g[u][1] = live[u] ? load4<T>(reinterpret_cast<const T*>(a.dkh) + src) : z;
          g[u][2] = live[u] ? load4<T>(reinterpret_cast<const T*>(a.dvh) + src) : z;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (live[u]) {
            store4<T>(reinterpret_cast<T*>(a.dq) + (size_t)m * a.ldq + c[u], g[u][0]);
            store4<T>(reinterpret_cast<T*>(a.dk) + (size_t)m * a.ldk + c[u], g[u][1]);
            store4<T>(reinterpret_cast<T*>(a.dv) + (size_t)m * a.ldv + c[u], g[u][2]);
          }
        }
      }
    } else {
      for (int p0 = 0; p0 < HP; p0 += 256) {
        const int pc = p0 + lane * 4;
        const int h = pc / DP, j = pc % DP;
        const bool live = pc < HP && j < a.d;
        const int c = h * a.d + j;
        const size_t src = (((size_t)b * a.H + h) * a.T + t) * DP + j;
        const f32x4 gq = live ? load4<T>(reinterpret_cast<const T*>(a.dqh) + src) : z;
        const f32x4 gk = live ? load4<T>(reinterpret_cast<const T*>(a.dkh) + src) : z;
        const f32x4 s = live ? load4<float>(s_row + c) : z, sinv = live ? load4<float>(sinv_row + c) : z;
        const f32x4 nq = live ? load4<T>(reinterpret_cast<const T*>(a.qh) + src) * sinv : z;   // unit vector
        const f32x4 nk = live ? load4<T>(reinterpret_cast<const T*>(a.kh) + src) * sinv : z;
        const f32x4 sgq = gq * s, sgk = gk * s;
        const float dq_ = group_sum<DP / 4>(a.d == DP ? dot4_sum(sgq, nq) : dot4_fma(sgq, nq));
        const float dk_ = group_sum<DP / 4>(dot4_fma(sgk, nk));
        if (live) {
          f32x4* r = reinterpret_cast<f32x4*>(red + c);   // this lane alone owns columns c..c+3 of the wave's row
          *r = *r + (gq * nq + gk * nk);
          const float rq = a.rq[(size_t)m * a.H + h], rk = a.rk[(size_t)m * a.H + h];
          store4<T>(reinterpret_cast<T*>(a.dq) + (size_t)m * a.ldq + c, (sgq - nq * dq_) * rq);
          store4<T>(reinterpret_cast<T*>(a.dk) + (size_t)m * a.ldk + c, (sgk - nk * dk_) * rk);
          store4<T>(reinterpret_cast<T*>(a.dv) + (size_t)m * a.ldv + c, load4<T>(reinterpret_cast<const T*>(a.dvh) + src));
        }
      }
    }
  }
  if constexpr (NORM) {
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < ROW_WAVES; ++w) t += merge_red[w * C + c];
      a.part[(size_t)blockIdx.x * C + c] = t;
    }
  }
}

// pad_cols_kernel: dst [M, H*PAD_D] = src [M, H*d] with zero pads (dO, and O rebuilt for the dQ kernel's delta);
// unpad_cols_kernel: dst [M, H*d] = the first d columns of every head of src [M, H*PAD_D] (O for the output projection).
// One thread per group of 4 destination elements.
template <typename T>
__global__ __launch_bounds__(256) void pad_cols_kernel(const T* src, T* dst, int M, int H, int d) {
  const size_t G = (size_t)H * (PAD_D / 4), total = (size_t)M * G;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
    const size_t m = g / G;
    const int pc = (int)(g % G) * 4, h = pc / PAD_D, j = pc % PAD_D;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    store4<T>(dst + g * 4, j < d ? load4<T>(src + m * ((size_t)H * d) + h * d + j) : z);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void unpad_cols_kernel(const T* src, T* dst, int M, int H, int d) {
  const size_t G = (size_t)H * d / 4, total = (size_t)M * G;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
    const size_t m = g / G;
    const int c = (int)(g % G) * 4, h = c / d, j = c % d;
    store4<T>(dst + g * 4, load4<T>(src + m * ((size_t)H * PAD_D) + h * PAD_D + j));
  }
}

// ------------------------------------------------------------------------------ SwiGLU
// thread owns 4 consecutive output columns j..j+3 (inside one 16-group), loops over a row range.
template <typename TI, typename T>   // TI: type of the pre-activations read, T: type of the gated output
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const TI* uv, const float* suv, float gscale, T* x, int M,
                                                          int F, int rows_per_blk) {
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= F) return;
  const int q = j >> 4, w = j & 15;
  const f32x4 one = {1.f, 1.f, 1.f, 1.f};
  const f32x4 gu = suv ? *reinterpret_cast<const f32x4*>(suv + j) * gscale : one;
  const f32x4 gv = suv ? *reinterpret_cast<const f32x4*>(suv + F + j) * gscale : one;
  const int r0 = blockIdx.y * rows_per_blk;
  const int r1 = min(M, r0 + rows_per_blk);
  for (int m = r0; m < r1; ++m) {
    const TI* row = uv + (size_t)m * 2 * F + q * 32 + w;
    const f32x4 u = load4<TI>(row) * gu;
    const f32x4 v = load4<TI>(row + 16) * gv;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = u[e] * (v[e] * sigmoidf_(v[e]));
    store4<T>(x + (size_t)m * F + j, o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* dx, const T* uv, const float* suv, float gscale,
                                                          T* duv, float* part, int M, int F, int rows_per_blk) {
  const int j = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (j >= F) return;
  const int q = j >> 4, w = j & 15;
  const f32x4 one = {1.f, 1.f, 1.f, 1.f};
  const f32x4 gu = suv ? *reinterpret_cast<const f32x4*>(suv + j) * gscale : one;
  const f32x4 gv = suv ? *reinterpret_cast<const f32x4*>(suv + F + j) * gscale : one;
  f32x4 dgu = {0.f, 0.f, 0.f, 0.f}, dgv = {0.f, 0.f, 0.f, 0.f};
  const int r0 = blockIdx.y * rows_per_blk;
  const int r1 = min(M, r0 + rows_per_blk);
  for (int m = r0; m < r1; ++m) {
    const size_t off = (size_t)m * 2 * F + q * 32 + w;
    const f32x4 ur = load4<T>(uv + off), vr = load4<T>(uv + off + 16);
    const f32x4 g = load4<T>(dx + (size_t)m * F + j);
    const f32x4 u = ur * gu, v = vr * gv;
    f32x4 du, dv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float sg = sigmoidf_(v[e]);
      du[e] = g[e] * v[e] * sg;
      dv[e] = g[e] * u[e] * sg * (1.0f + v[e] * (1.0f - sg));
    }
    dgu += du * ur;
    dgv += dv * vr;
    store4<T>(duv + off, du * gu);
    store4<T>(duv + off + 16, dv * gv);
  }
  if (part) {
    float* p = part + (size_t)blockIdx.y * 2 * F;
    *reinterpret_cast<f32x4*>(p + j) = dgu * gscale;
    *reinterpret_cast<f32x4*>(p + F + j) = dgv * gscale;
  }
}

// ------------------------------------------------------------------------------ small reductions
// out[n] = f(sum_b part[b][n]); 1024 threads = 32 columns x 32 row groups, fixed summation order (the partial arrays
// are a few MB and there are only N/32 workgroups, so the kernel is latency-bound: many short rows per thread)
constexpr int CSR_RG = 32;
__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const float* part, int nblk, int N, float* out,
                                                              int accumulate, int kind, const float* ref, float scale) {
  __shared__ float red[CSR_RG][33];
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int n = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (n < N) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = rg;
    for (; b + 3 * CSR_RG < nblk; b += 4 * CSR_RG) {
      s0 += part[(size_t)b * N + n];
      s1 += part[(size_t)(b + CSR_RG) * N + n];
      s2 += part[(size_t)(b + 2 * CSR_RG) * N + n];
      s3 += part[(size_t)(b + 3 * CSR_RG) * N + n];
    }
    for (; b < nblk; b += CSR_RG) s0 += part[(size_t)b * N + n];
    s = (s0 + s1) + (s2 + s3);
  }
  red[rg][cl] = s;
  __syncthreads();
  if (rg != 0 || n >= N) return;
#pragma unroll
  for (int g = 1; g < CSR_RG; ++g) s += red[g][cl];
  if (kind == 1) {
    const float r = ref[n] * scale;
    s = s * (r > 0.f ? scale : (r < 0.f ? -scale : 0.f));
  } else {
    s *= scale;
  }
  int dst = n;
  if (kind == 2) {
    const int q = n >> 5, w = n & 31, F = N >> 1;
    dst = w < 16 ? q * 16 + w : F + q * 16 + (w - 16);
  }
  out[dst] = accumulate ? out[dst] + s : s;
}

// Several reductions of the kind above in ONE launch (the six parameter-gradient reductions of a block's backward were
// six ~12 us launches on the critical stream, 0.9 ms per Base step).  An item may have a second partial array whose
// reduced, scaled sum is added after the first one's (fixed order: e.g. the q and k contributions to d sqk).
constexpr int CSR_MAX_ITEMS = NVIT_COLSUM_REDUCE_MAX_ITEMS;
struct CsrItem {
  const float* part;
  const float* part_b;   // optional second partial array (same N), or NULL
  const float* ref;
  float* out;
  int nblk, nblk_b, N, accumulate, kind, block0;   // block0: first workgroup of this item in the launch
  float scale;
};
struct CsrBatch {
  CsrItem it[CSR_MAX_ITEMS];
  int n;
};

__device__ __forceinline__ float csr_column(const float* part, int nblk, int N, int n, int rg) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int b = rg;
  for (; b + 3 * CSR_RG < nblk; b += 4 * CSR_RG) {
    s0 += part[(size_t)b * N + n];
    s1 += part[(size_t)(b + CSR_RG) * N + n];
    s2 += part[(size_t)(b + 2 * CSR_RG) * N + n];
    s3 += part[(size_t)(b + 3 * CSR_RG) * N + n];
  }
  for (; b < nblk; b += CSR_RG) s0 += part[(size_t)b * N + n];
  return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(1024) void colsum_reduce_multi_kernel(CsrBatch bt) {
  __shared__ float red[2][CSR_RG][33];
  int k = 0;
#pragma unroll
  for (int i = 1; i < CSR_MAX_ITEMS; ++i)
    if (i < bt.n && (int)blockIdx.x >= bt.it[i].block0) k = i;
  // (copy of the selected item through a uniform index: the struct lives in kernel-argument memory)
  const float* part = bt.it[k].part;
  const float* part_b = bt.it[k].part_b;
  const float* ref = bt.it[k].ref;
  float* out = bt.it[k].out;
  const int nblk = bt.it[k].nblk, nblk_b = bt.it[k].nblk_b, N = bt.it[k].N, accumulate = bt.it[k].accumulate,
            kind = bt.it[k].kind, blk = (int)blockIdx.x - bt.it[k].block0;
  const float scale = bt.it[k].scale;
  const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int n = blk * 32 + cl;
  red[0][rg][cl] = n < N ? csr_column(part, nblk, N, n, rg) : 0.f;
  red[1][rg][cl] = (n < N && part_b) ? csr_column(part_b, nblk_b, N, n, rg) : 0.f;
  __syncthreads();
  if (rg != 0 || n >= N) return;
  float s = red[0][0][cl], sb = red[1][0][cl];
#pragma unroll
  for (int g = 1; g < CSR_RG; ++g) {
    s += red[0][g][cl];
    sb += red[1][g][cl];
  }
  if (kind == 1) {
    const float r = ref[n] * scale;
    const float f = r > 0.f ? scale : (r < 0.f ? -scale : 0.f);
    s = s * f;
    sb = sb * f;
  } else {
    s *= scale;
    sb *= scale;
  }
  int dst = n;
  if (kind == 2) {
    const int q = n >> 5, w = n & 31, F = N >> 1;
    dst = w < 16 ? q * 16 + w : F + q * 16 + (w - 16);
  }
  float r = accumulate ? out[dst] + s : s;
  if (part_b) r += sb;
  out[dst] = r;
}

template <typename TA, typename TB>
__global__ void colsum_kernel(const TA* a, int lda, const TB* b, int ldb, int R, int N, int period, float* out,
                              int accumulate, float scale) {
  // one thread per output element (row class rc in [0,period), column n); loops rows r = rc, rc+period, ...
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int rc = blockIdx.y;
  if (n >= N) return;
  // four independent partial sums (fixed order): four loads in flight per thread instead of a dependent chain
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int r = rc;
  for (; r + 3 * period < R; r += 4 * period) {
    float v0 = ld1<TA>(a + (size_t)r * lda + n);
    float v1 = ld1<TA>(a + (size_t)(r + period) * lda + n);
    float v2 = ld1<TA>(a + (size_t)(r + 2 * period) * lda + n);
    float v3 = ld1<TA>(a + (size_t)(r + 3 * period) * lda + n);
    if (b) {
      v0 *= ld1<TB>(b + (size_t)r * ldb + n);
      v1 *= ld1<TB>(b + (size_t)(r + period) * ldb + n);
      v2 *= ld1<TB>(b + (size_t)(r + 2 * period) * ldb + n);
      v3 *= ld1<TB>(b + (size_t)(r + 3 * period) * ldb + n);
    }
    s0 += v0;
    s1 += v1;
    s2 += v2;
    s3 += v3;
  }
  for (; r < R; r += period) {
    float v = ld1<TA>(a + (size_t)r * lda + n);
    if (b) v *= ld1<TB>(b + (size_t)r * ldb + n);
    s0 += v;
  }
  float s = ((s0 + s1) + (s2 + s3)) * scale;
  float* o = out + (size_t)rc * N + n;
  *o = accumulate ? *o + s : s;
}

template <typename T>
__global__ void cast_kernel(const float* src, T* dst, long long n4) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
    store4<T>(dst + i * 4, *reinterpret_cast<const f32x4*>(src + i * 4));
}

template <typename T>
__global__ void scale_cols_kernel(const float* a, int lda, const float* s, float c, T* out, int ldo, int R, int N) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (n >= N || r >= R) return;
  st1<T>(out + (size_t)r * ldo + n, s ? a[(size_t)r * lda + n] * s[n] * c : a[(size_t)r * lda + n] * c);
}

// Input pipeline, deterministic part (reference train.py:1084-1090): ToTensor (uint8 HWC -> float CHW in [0,1]) and
// kornia Normalize(mean 0.5, std 0.5) in one pass: out[b,c,y,x] = (in/255 - mean) / std.  IN = uint8 (HWC, one byte per
// channel) or float (CHW, already in [0,1]).  Four output pixels per thread, 16-byte stores.
template <typename IN>
__global__ void normalize_images_kernel(const IN* in, float* out, int B, int C, int H, int W, float mean, float inv_std) {
  const long long n4 = (long long)B * C * H * (W / 4);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const int x4 = (int)(i % (W / 4)) * 4;
    long long r = i / (W / 4);
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C), b = (int)(r / C);
    f32x4 v;
    if constexpr (sizeof(IN) == 1) {
      const IN* p = in + (((size_t)b * H + y) * W + x4) * C + c;   // HWC
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)p[(size_t)e * C] * (1.0f / 255.0f);
    } else {
      v = *reinterpret_cast<const f32x4*>(in + (((size_t)b * C + c) * H + y) * W + x4);
    }
    *reinterpret_cast<f32x4*>(out + (((size_t)b * C + c) * H + y) * W + x4) = (v - mean) * inv_std;
  }
}

// ------------------------------------------------------------------------------ RMSNorm (reference model.py:170-182)
// y = x * rsqrt(mean(x^2) + eps) * w.  Dead on the nViT path (its Block never calls it); kept as a working public module.
template <int NV>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const float* x, const float* w, float eps, float* out,
                                                           float* rstd, int M, int C) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  RowVec<NV> wv;
  row_load<NV, float>(wv, w, C, lane);
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> a;
    row_load<NV, float>(a, x + (size_t)m * C, C, lane);
    const float rs = 1.0f / sqrtf(row_dot<NV>(a, a) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) a.v[i] = a.v[i] * rs * wv.v[i];
    row_store<NV, float>(a, out + (size_t)m * C, C, lane);
    if (lane == 0) rstd[m] = rs;
  }
}

// dx = rstd * (g*w - xn * mean(g*w*xn)),  xn = x * rstd;  part_dw[block][c] = sum over the block's rows of g * xn
template <int NV>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const float* dout, const float* x, const float* w,
                                                           const float* rstd, float* dx, float* part_dw, int M, int C) {
  __shared__ float red[ROW_WAVES][NV * 256];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  RowVec<NV> wv, dw;
  row_load<NV, float>(wv, w, C, lane);
#pragma unroll
  for (int i = 0; i < NV; ++i) dw.v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int m = blockIdx.x * ROW_WAVES + wid; m < M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> a, g;
    row_load<NV, float>(a, x + (size_t)m * C, C, lane);
    row_load<NV, float>(g, dout + (size_t)m * C, C, lane);
    const float rs = rstd[m];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      a.v[i] = a.v[i] * rs;            // xn
      dw.v[i] += g.v[i] * a.v[i];
      g.v[i] = g.v[i] * wv.v[i];       // g*w
    }
    const float mean = row_dot<NV>(g, a) / (float)C;
#pragma unroll
    for (int i = 0; i < NV; ++i) g.v[i] = (g.v[i] - a.v[i] * mean) * rs;
    row_store<NV, float>(g, dx + (size_t)m * C, C, lane);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[wid][(i * 64 + lane) * 4 + e] = dw.v[i][e];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s_ = 0.f;
#pragma unroll
    for (int wv_ = 0; wv_ < ROW_WAVES; ++wv_) s_ += red[wv_][c];
    part_dw[(size_t)blockIdx.x * C + c] = s_;
  }
}

// ------------------------------------------------------------------------------ residual + RMSNorm (plain-ViT blocks)
// The use_nvit=False Block (reference model.py:92-169 with the RMSNorm modules built): a = rms_att(x);
// h1 = a + attn(a); bm = rms_mlp(h1); h2 = bm + mlp(bm); then norm_skip: out = nrm(h2*skip + x).
// res_rmsnorm_fwd: out = rms(a + y) * w (y = NULL: rms(a) * w), with the operand twin and rstd; a + y is not stored.
struct ResRmsFwdArgs {
  const float* a;
  const void* y;
  const float* w;
  float eps;
  float* out;
  void* out_lo;
  float* rstd;
  int M, C;
  const float* gate;   // GATED kernels: one fp32 gate per sample (DropPath), T rows per sample
  int T;
};

// GATED (stochastic depth of the plain-ViT blocks, with HAS_Y): z = a + gate * y, the gate folded into y where it is loaded.
template <int NV, typename TY, typename TL, bool HAS_Y, bool GATED>
__global__ __launch_bounds__(256) void res_rmsnorm_fwd_kernel(ResRmsFwdArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  RowVec<NV> wv;
  row_load<NV, float>(wv, a.w, a.C, lane);
  for (int m = blockIdx.x * ROW_WAVES + wid; m < a.M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> z;
    row_load<NV, float>(z, a.a + (size_t)m * a.C, a.C, lane);
    if constexpr (HAS_Y) {
      RowVec<NV> y;
      row_load<NV, TY>(y, reinterpret_cast<const TY*>(a.y) + (size_t)m * a.C, a.C, lane);
      if constexpr (GATED) {
        const float gt = row_gate(a.gate, m, a.T);
#pragma unroll
        for (int i = 0; i < NV; ++i) y.v[i] = y.v[i] * gt;
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) z.v[i] = z.v[i] + y.v[i];
    }
    const float rs = 1.0f / sqrtf(row_dot<NV>(z, z) / (float)a.C + a.eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) z.v[i] = z.v[i] * rs * wv.v[i];
    row_store<NV, float>(z, a.out + (size_t)m * a.C, a.C, lane);
    if (a.out_lo) row_store<NV, TL>(z, reinterpret_cast<TL*>(a.out_lo) + (size_t)m * a.C, a.C, lane);
    if (lane == 0) a.rstd[m] = rs;
  }
}

// res_rmsnorm_bwd: gradient g (+ the addend g_add of type TL: a data-gradient GEMM's output) of out = rms(z) * w,
// z = a + y, recomputed.  dz = rstd * (gw - zn * mean(gw * zn)), gw = g * w, zn = z * rstd; written (or added to dz with
// accum), its type-TL copy to dz_lo; per-wave partial sums part_dw [4*nblk, C] of g * zn.
struct ResRmsBwdArgs {
  const float* g;
  const void* g_add;
  const float* a;
  const void* y;
  const float* w;
  const float* rstd;
  float* dz;
  int accum;
  void* dz_lo;
  float* part_dw;
  int M, C;
  const float* gate;   // GATED kernels: as in ResRmsFwdArgs
  int T;
};

// GATED: z = a + gate * y as in the forward.  dz (fp32) stays d(z), the gradient that goes on down the stream into a; the
// type-TL copy dz_lo is gate * d(z) = d(y), what the branch's GEMMs read - with a gate the two are different tensors in
// fp32 mode too.
template <int NV, typename TY, typename TL, bool HAS_Y, bool ADD, bool GATED>
__global__ __launch_bounds__(256) void res_rmsnorm_bwd_kernel(ResRmsBwdArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  RowVec<NV> wv, dw;
  row_load<NV, float>(wv, a.w, a.C, lane);
#pragma unroll
  for (int i = 0; i < NV; ++i) dw.v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int m = blockIdx.x * ROW_WAVES + wid; m < a.M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> z, g;
    row_load<NV, float>(z, a.a + (size_t)m * a.C, a.C, lane);
    row_load_f32_nt<NV>(g, a.g + (size_t)m * a.C, a.C, lane);
    float gt = 1.0f;
    if constexpr (GATED) gt = row_gate(a.gate, m, a.T);
    if constexpr (HAS_Y) {
      RowVec<NV> y;
      row_load<NV, TY>(y, reinterpret_cast<const TY*>(a.y) + (size_t)m * a.C, a.C, lane);
      if constexpr (GATED) {
#pragma unroll
        for (int i = 0; i < NV; ++i) y.v[i] = y.v[i] * gt;
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) z.v[i] = z.v[i] + y.v[i];
    }
    if constexpr (ADD) {
      RowVec<NV> ad;
      row_load<NV, TL>(ad, reinterpret_cast<const TL*>(a.g_add) + (size_t)m * a.C, a.C, lane);
#pragma unroll
      for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] + ad.v[i];
    }
    const float rs = a.rstd[m];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      z.v[i] = z.v[i] * rs;            // zn
      dw.v[i] += g.v[i] * z.v[i];
      g.v[i] = g.v[i] * wv.v[i];       // gw
    }
    const float mean = row_dot<NV>(g, z) / (float)a.C;
#pragma unroll
    for (int i = 0; i < NV; ++i) g.v[i] = (g.v[i] - z.v[i] * mean) * rs;
    float* dz = a.dz + (size_t)m * a.C;
    if (a.accum) {
      RowVec<NV> old;
      row_load<NV, float>(old, dz, a.C, lane);
#pragma unroll
      for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] + old.v[i];
    }
    row_store<NV, float>(g, dz, a.C, lane);
    if constexpr (GATED) {
#pragma unroll
      for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] * gt;
    }
    if (a.dz_lo) row_store<NV, TL>(g, reinterpret_cast<TL*>(a.dz_lo) + (size_t)m * a.C, a.C, lane);
  }
  row_store<NV, float>(dw, a.part_dw + ((size_t)blockIdx.x * ROW_WAVES + wid) * a.C, a.C, lane);
}

// res_skip_fwd: out = nrm((h + y) * skip + x)  (norm_skip after a plain-ViT block, reference model.py:84-87,450-452).
struct ResSkipArgs {
  const float* dout;
  const float* h;
  const void* y;
  const float* skip;
  const float* x;
  float* out;      // fwd: the new stream; bwd: d(x) (written)
  void* out_lo;    // fwd: its type-TL twin; bwd: the type-TL copy of d(h + y) (may be NULL)
  float* dh;       // bwd: d(h + y), fp32
  float* part_dskip;
  int M, C;
  const float* gate;   // GATED kernels: as in ResRmsFwdArgs
  int T;
};

// GATED: out = nrm((h + gate * y) * skip + x), the gate folded into y where it is loaded.
template <int NV, typename TY, typename TL, bool GATED>
__global__ __launch_bounds__(256) void res_skip_fwd_kernel(ResSkipArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float sk = a.skip[0];
  for (int m = blockIdx.x * ROW_WAVES + wid; m < a.M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> r, y, x;
    row_load<NV, float>(r, a.h + (size_t)m * a.C, a.C, lane);
    row_load<NV, TY>(y, reinterpret_cast<const TY*>(a.y) + (size_t)m * a.C, a.C, lane);
    row_load<NV, float>(x, a.x + (size_t)m * a.C, a.C, lane);
    if constexpr (GATED) {
      const float gt = row_gate(a.gate, m, a.T);
#pragma unroll
      for (int i = 0; i < NV; ++i) y.v[i] = y.v[i] * gt;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = (r.v[i] + y.v[i]) * sk + x.v[i];
    const float rs = 1.0f / sqrtf(row_dot<NV>(r, r));
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = r.v[i] * rs;
    row_store<NV, float>(r, a.out + (size_t)m * a.C, a.C, lane);
    if (a.out_lo) row_store<NV, TL>(r, reinterpret_cast<TL*>(a.out_lo) + (size_t)m * a.C, a.C, lane);
  }
}

// res_skip_bwd: dr = (g - o (o.g)) / |r|;  d(x) = dr,  d(h + y) = dr * skip,  part_dskip [4*nblk] = per-wave sums of
// dr . (h + y).  GATED: h + gate * y throughout; dh (fp32) stays d(h + gate * y), the gradient that goes on into h, and its
// type-TL copy is gate * dh = d(y), what the branch's GEMMs read (see res_rmsnorm_bwd_kernel).
template <int NV, typename TY, typename TL, bool GATED>
__global__ __launch_bounds__(256) void res_skip_bwd_kernel(ResSkipArgs a) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float sk = a.skip[0];
  float acc = 0.f;
  for (int m = blockIdx.x * ROW_WAVES + wid; m < a.M; m += gridDim.x * ROW_WAVES) {
    RowVec<NV> s, y, r, g;
    row_load<NV, float>(s, a.h + (size_t)m * a.C, a.C, lane);
    row_load<NV, TY>(y, reinterpret_cast<const TY*>(a.y) + (size_t)m * a.C, a.C, lane);
    row_load<NV, float>(r, a.x + (size_t)m * a.C, a.C, lane);
    row_load_f32_nt<NV>(g, a.dout + (size_t)m * a.C, a.C, lane);
    float gt = 1.0f;
    if constexpr (GATED) {
      gt = row_gate(a.gate, m, a.T);
#pragma unroll
      for (int i = 0; i < NV; ++i) y.v[i] = y.v[i] * gt;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      s.v[i] = s.v[i] + y.v[i];
      r.v[i] = s.v[i] * sk + r.v[i];
    }
    const float rs = 1.0f / sqrtf(row_dot<NV>(r, r));
#pragma unroll
    for (int i = 0; i < NV; ++i) r.v[i] = r.v[i] * rs;   // o
    const float og = row_dot<NV>(r, g);
#pragma unroll
    for (int i = 0; i < NV; ++i) g.v[i] = (g.v[i] - r.v[i] * og) * rs;   // dr
    acc += row_dot<NV>(g, s);
    row_store<NV, float>(g, a.out + (size_t)m * a.C, a.C, lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] * sk;
    row_store<NV, float>(g, a.dh + (size_t)m * a.C, a.C, lane);
    if constexpr (GATED) {
#pragma unroll
      for (int i = 0; i < NV; ++i) g.v[i] = g.v[i] * gt;
    }
    if (a.out_lo) row_store<NV, TL>(g, reinterpret_cast<TL*>(a.out_lo) + (size_t)m * a.C, a.C, lane);
  }
  if (lane == 0) a.part_dskip[(size_t)blockIdx.x * ROW_WAVES + wid] = acc;
}

int row_grid(int M) {
  const int blocks = cdiv(M, ROW_WAVES);
  return blocks > NVIT_ROW_GRID_MAX ? NVIT_ROW_GRID_MAX : blocks;
}

}  // namespace

// ---- run-time options -> template instantiation.  Each family picks its kernel in ONE selector built from dispatch.h; the
// entry points launch through the pointer it returns (families whose kernels take typed pointers launch inside it). ----

// (NV, TY, TL) of the row kernels that read y as y_dt and write their low-precision copy as dt
template <typename F>
static auto with_row_types(int C, int y_dt, int dt, F&& f) {
  return with_row_vecs<8>(C, [&](auto nv) {
    return with_elem(y_dt, [&](auto ty) { return with_elem(dt, [&](auto tl) { return f(nv, ty, tl); }); });
  });
}

// (type read, type written) of a dt that may be NVIT_BF16_F32IN: fp32 in, bf16 out, computed from the unrounded values
template <typename F>
static auto with_in_out_elems(int dt, F&& f) {
  if (dt == NVIT_F32) return f(type_tag<float>{}, type_tag<float>{});
  if (dt == NVIT_BF16) return f(type_tag<bf16>{}, type_tag<bf16>{});
  return f(type_tag<float>{}, type_tag<bf16>{});
}

// The lerp_bwd instantiation for a call's options: nvit_lerp_bwd launches it and nvit_lerp_bwd_blocks sizes that launch's
// grid from its occupancy, so both go through here.  The gated instantiations are the two the block chain of ViT.forward
// launches: the MLP half (norm_skip fused, dh written) and the attention half (no skip, dh accumulated), each with and
// without the bf16 addend; both callers refuse a gated call with has_skip == accum before they come here.
static auto lerp_bwd_select(int C, int y_dt, int dt, bool has_add, bool has_skip, bool accum, bool gated) -> void (*)(LerpBwdArgs) {
  return with_row_types(C, y_dt, dt, [&](auto nv, auto ty, auto tl) {
    return with_bool(has_add, [&](auto add) {
      using TY = tag_t<decltype(ty)>;
      using TL = tag_t<decltype(tl)>;
      if (gated && has_skip) return &lerp_bwd_kernel<nv, TY, TL, add, true, false, true>;
      if (gated) return &lerp_bwd_kernel<nv, TY, TL, add, false, true, true>;
      return with_bool(has_skip, [&](auto skip) {
        return with_bool(accum, [&](auto acc) { return &lerp_bwd_kernel<nv, TY, TL, add, skip, acc, false>; });
      });
    });
  });
}

// ---- the gate of stochastic depth, optional in the six entry points below: NULL launches the GATED = false instantiation
// (rows_per_sample is then ignored), a gate the GATED = true one, which reads one float per sample on top of the rows. ----
static bool gate_args_ok(const float* gate, int rows_per_sample, int M) {
  return !gate || (rows_per_sample > 0 && M % rows_per_sample == 0);
}
static double gate_bytes(const float* gate, int M) { return gate ? 4.0 * M : 0.0; }
static double elem_bytes(int dt) { return dt == NVIT_F32 ? 4.0 : 2.0; }

extern "C" int nvit_lerp_fwd(int dt, const float* h, const void* y, int y_dt, const float* alpha, float c_a,
                             const float* skip_x, const float* skip, const float* gate, int rows_per_sample, float* out,
                             void* out_lo, int M, int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "lerp_fwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  NVIT_REQUIRE(!skip_x || skip, "lerp_fwd: skip_x without skip");
  NVIT_REQUIRE(gate_args_ok(gate, rows_per_sample, M), "lerp_fwd: with a gate, M=%d must be a multiple of rows_per_sample=%d", M,
               rows_per_sample);
  LerpFwdArgs a{h, y, alpha, c_a, skip_x, skip, out, out_lo, M, C, gate, gate ? rows_per_sample : 1};
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * C * (skip_x ? 16.0 : 12.0) + gate_bytes(gate, M), s);
  const auto kernel = with_row_types(C, y_dt, dt, [&](auto nv, auto ty, auto tl) {
    return with_bool(gate != nullptr, [&](auto gated) { return &lerp_fwd_kernel<nv, tag_t<decltype(ty)>, tag_t<decltype(tl)>, gated>; });
  });
  launch(kernel, dim3(row_grid(M)), dim3(256), 0, s, a);
  NVIT_CHECK_LAUNCH("lerp_fwd");
  return NVIT_OK;
}

// Workgroups that are resident at once for the lerp_bwd instantiation a call with these options would launch (CUs x
// blocks per CU from the occupancy query).  The kernel walks its rows with a grid stride, so a grid of exactly this many
// blocks keeps every SIMD busy to the end; the round-2 default of 1024 blocks ran as 768 + 256 at C = 768 (3 waves per
// SIMD): a second, one-third-full round (row kernels 14.9 -> 13.1 ms per Base step with the resident count).
static int resident_blocks(void (*kernel)(LerpBwdArgs)) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) return 0;
  return per_cu * nvit_num_cu();
}

extern "C" int nvit_lerp_bwd_blocks(int dt, int y_dt, int C, int has_add, int has_skip, int accum, int gated) {
  if (C % 4 != 0 || C <= 0 || C > NVIT_MAX_EMBD || (gated && (has_skip != 0) == (accum != 0))) return 0;
  const int n = resident_blocks(lerp_bwd_select(C, y_dt, dt, has_add, has_skip, accum, gated));
  return n > NVIT_MAX_PART_BLOCKS ? NVIT_MAX_PART_BLOCKS : n;
}

extern "C" int nvit_lerp_bwd(int dt, const float* dout, const void* dout_add, const float* h, const void* y, int y_dt, const float* alpha,
                             float c_a, const float* skip_x, const float* skip, const float* gate, int rows_per_sample,
                             float* dh, int accum_dh, float* dy, void* dy_lo, float* dskip_x, float* part_dlam,
                             float* part_dskip, int nblk, int M, int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "lerp_bwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  NVIT_REQUIRE(nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "lerp_bwd: nblk out of range");
  NVIT_REQUIRE(!skip_x || (skip && dskip_x && part_dskip), "lerp_bwd: skip buffers missing");
  NVIT_REQUIRE(gate_args_ok(gate, rows_per_sample, M), "lerp_bwd: with a gate, M=%d must be a multiple of rows_per_sample=%d", M,
               rows_per_sample);
  NVIT_REQUIRE(!gate || (skip_x != nullptr) != (accum_dh != 0),
               "lerp_bwd: with a gate, built for the two calls of the block chain, skip_x without accum_dh or accum_dh without skip_x");
  LerpBwdArgs a{dout, (const bf16*)dout_add, h, y, alpha, c_a, skip_x, skip, dh, accum_dh, dy, dy_lo, dskip_x, part_dlam, part_dskip, M, C, gate, gate ? rows_per_sample : 1};
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: dout, h read, y read (2 or 4 B), dh written, dy_lo written (+ skip_x read, dskip_x written; + dout_add)
  const double lb_bytes = (double)M * C * (4.0 + 4.0 + elem_bytes(y_dt) + 4.0 + (dy ? 4.0 : 0.0) + (dy_lo ? elem_bytes(dt) : 0.0) +
                                           (skip_x ? 8.0 : 0.0) + (accum_dh ? 4.0 : 0.0) + (dout_add ? 2.0 : 0.0)) + gate_bytes(gate, M);
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, lb_bytes, s);
  launch(lerp_bwd_select(C, y_dt, dt, dout_add != nullptr, skip_x != nullptr, accum_dh != 0, gate != nullptr), dim3(nblk), dim3(256), 0, s, a);
  NVIT_CHECK_LAUNCH("lerp_bwd");
  return NVIT_OK;
}

extern "C" int nvit_norm_skip_fwd(const float* src, const float* tgt, const float* skip, float* out, int M, int C,
                                  void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "norm_skip_fwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  hipStream_t s = (hipStream_t)stream;
  const int grid = row_grid(M);
  with_row_vecs<8>(C, [&](auto nv) { launch(norm_skip_fwd_kernel<nv>, dim3(grid), dim3(256), 0, s, src, tgt, skip, out, M, C); });
  NVIT_CHECK_LAUNCH("norm_skip_fwd");
  return NVIT_OK;
}

extern "C" int nvit_norm_skip_bwd(const float* dout, const float* src, const float* tgt, const float* skip, float* dsrc,
                                  float* dtgt, float* part_dskip, int nblk, int M, int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0 && nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "norm_skip_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  with_row_vecs<8>(C, [&](auto nv) {
    launch(norm_skip_bwd_kernel<nv>, dim3(nblk), dim3(256), 0, s, dout, src, tgt, skip, dsrc, dtgt, part_dskip, M, C);
  });
  NVIT_CHECK_LAUNCH("norm_skip_bwd");
  return NVIT_OK;
}

extern "C" int nvit_rmsnorm_fwd(const float* x, const float* w, float eps, float* out, float* rstd, int M, int C,
                                void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "rmsnorm_fwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  hipStream_t s = (hipStream_t)stream;
  const int grid = row_grid(M);
  with_row_vecs<8>(C, [&](auto nv) { launch(rmsnorm_fwd_kernel<nv>, dim3(grid), dim3(256), 0, s, x, w, eps, out, rstd, M, C); });
  NVIT_CHECK_LAUNCH("rmsnorm_fwd");
  return NVIT_OK;
}

extern "C" int nvit_rmsnorm_bwd(const float* dout, const float* x, const float* w, const float* rstd, float* dx,
                                float* part_dw, int nblk, int M, int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0 && nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "rmsnorm_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  with_row_vecs<8>(C, [&](auto nv) {
    launch(rmsnorm_bwd_kernel<nv>, dim3(nblk), dim3(256), 0, s, dout, x, w, rstd, dx, part_dw, M, C);
  });
  NVIT_CHECK_LAUNCH("rmsnorm_bwd");
  return NVIT_OK;
}

// ---- residual kernels of the plain-ViT block chain.  The gated instantiations are built for the calls _StdBlockFn makes:
// a branch output y is always there, the rms_mlp backward always has its data-gradient addend. ----
extern "C" int nvit_res_rmsnorm_fwd(int dt, const float* a, const void* y, int y_dt, const float* w, float eps,
                                    const float* gate, int rows_per_sample, float* out, void* out_lo, float* rstd, int M,
                                    int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "res_rmsnorm_fwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "res_rmsnorm_fwd: bad dt %d", dt);
  NVIT_REQUIRE(!y || y_dt == NVIT_F32 || y_dt == NVIT_BF16, "res_rmsnorm_fwd: bad y_dt %d", y_dt);
  NVIT_REQUIRE(!gate || y, "res_rmsnorm_fwd: a gate needs y");
  NVIT_REQUIRE(gate_args_ok(gate, rows_per_sample, M), "res_rmsnorm_fwd: with a gate, M=%d must be a multiple of rows_per_sample=%d", M,
               rows_per_sample);
  ResRmsFwdArgs ar{a, y, w, eps, out, out_lo, rstd, M, C, gate, gate ? rows_per_sample : 1};
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * C * (8.0 + (y ? elem_bytes(y_dt) : 0.0) + (out_lo ? elem_bytes(dt) : 0.0)) +
                                         gate_bytes(gate, M), s);
  const auto kernel = with_row_vecs<8>(C, [&](auto nv) {
    return with_elem(dt, [&](auto tl) {
      using TL = tag_t<decltype(tl)>;
      if (!y) return &res_rmsnorm_fwd_kernel<nv, float, TL, false, false>;   // without y, TY is float: no <bf16, false> is built
      return with_elem(y_dt, [&](auto ty) {
        return with_bool(gate != nullptr, [&](auto gated) { return &res_rmsnorm_fwd_kernel<nv, tag_t<decltype(ty)>, TL, true, gated>; });
      });
    });
  });
  launch(kernel, dim3(row_grid(M)), dim3(256), 0, s, ar);
  NVIT_CHECK_LAUNCH("res_rmsnorm_fwd");
  return NVIT_OK;
}

extern "C" int nvit_res_rmsnorm_bwd(int dt, const float* g, const void* g_add, const float* a, const void* y, int y_dt,
                                    const float* w, const float* rstd, const float* gate, int rows_per_sample, float* dz,
                                    int accum, void* dz_lo, float* part_dw, int nblk, int M, int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "res_rmsnorm_bwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  NVIT_REQUIRE(nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "res_rmsnorm_bwd: nblk out of range");
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "res_rmsnorm_bwd: bad dt %d", dt);
  NVIT_REQUIRE(!y || y_dt == NVIT_F32 || y_dt == NVIT_BF16, "res_rmsnorm_bwd: bad y_dt %d", y_dt);
  NVIT_REQUIRE(!gate || y, "res_rmsnorm_bwd: a gate needs y");
  NVIT_REQUIRE(!gate || g_add, "res_rmsnorm_bwd: with a gate, built with the addend g_add only");
  NVIT_REQUIRE(gate_args_ok(gate, rows_per_sample, M), "res_rmsnorm_bwd: with a gate, M=%d must be a multiple of rows_per_sample=%d", M,
               rows_per_sample);
  ResRmsBwdArgs ar{g, g_add, a, y, w, rstd, dz, accum, dz_lo, part_dw, M, C, gate, gate ? rows_per_sample : 1};
  hipStream_t s = (hipStream_t)stream;
  const double tl = elem_bytes(dt);
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * C * (12.0 + (y ? elem_bytes(y_dt) : 0.0) + (g_add ? tl : 0.0) + (accum ? 4.0 : 0.0) +
                                                       (dz_lo ? tl : 0.0)) + gate_bytes(gate, M), s);
  const auto kernel = with_row_vecs<8>(C, [&](auto nv) {
    return with_elem(dt, [&](auto tlo) {
      using TL = tag_t<decltype(tlo)>;
      if (gate) return with_elem(y_dt, [&](auto ty) { return &res_rmsnorm_bwd_kernel<nv, tag_t<decltype(ty)>, TL, true, true, true>; });
      return with_bool(g_add != nullptr, [&](auto add) {
        if (!y) return &res_rmsnorm_bwd_kernel<nv, float, TL, false, add, false>;   // as in the forward: TY is float without y
        return with_elem(y_dt, [&](auto ty) { return &res_rmsnorm_bwd_kernel<nv, tag_t<decltype(ty)>, TL, true, add, false>; });
      });
    });
  });
  launch(kernel, dim3(nblk), dim3(256), 0, s, ar);
  NVIT_CHECK_LAUNCH("res_rmsnorm_bwd");
  return NVIT_OK;
}

extern "C" int nvit_res_skip_fwd(int dt, const float* h, const void* y, int y_dt, const float* skip, const float* x,
                                 const float* gate, int rows_per_sample, float* out, void* out_lo, int M, int C,
                                 void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "res_skip_fwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "res_skip_fwd: bad dt %d", dt);
  NVIT_REQUIRE(y && (y_dt == NVIT_F32 || y_dt == NVIT_BF16), "res_skip_fwd: y missing or bad y_dt %d", y_dt);
  NVIT_REQUIRE(gate_args_ok(gate, rows_per_sample, M), "res_skip_fwd: with a gate, M=%d must be a multiple of rows_per_sample=%d", M,
               rows_per_sample);
  ResSkipArgs ar{nullptr, h, y, skip, x, out, out_lo, nullptr, nullptr, M, C, gate, gate ? rows_per_sample : 1};
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * C * (12.0 + elem_bytes(y_dt) + (out_lo ? elem_bytes(dt) : 0.0)) + gate_bytes(gate, M), s);
  const auto kernel = with_row_types(C, y_dt, dt, [&](auto nv, auto ty, auto tl) {
    return with_bool(gate != nullptr, [&](auto gated) { return &res_skip_fwd_kernel<nv, tag_t<decltype(ty)>, tag_t<decltype(tl)>, gated>; });
  });
  launch(kernel, dim3(row_grid(M)), dim3(256), 0, s, ar);
  NVIT_CHECK_LAUNCH("res_skip_fwd");
  return NVIT_OK;
}

extern "C" int nvit_res_skip_bwd(int dt, const float* dout, const float* h, const void* y, int y_dt, const float* skip,
                                 const float* x, const float* gate, int rows_per_sample, float* dh, void* dh_lo, float* dx,
                                 float* part_dskip, int nblk, int M, int C, void* stream) {
  NVIT_REQUIRE(C % 4 == 0 && C <= NVIT_MAX_EMBD && M > 0, "res_skip_bwd: C=%d must be a multiple of 4 and <= %d", C, NVIT_MAX_EMBD);
  NVIT_REQUIRE(nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "res_skip_bwd: nblk out of range");
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "res_skip_bwd: bad dt %d", dt);
  NVIT_REQUIRE(y && (y_dt == NVIT_F32 || y_dt == NVIT_BF16), "res_skip_bwd: y missing or bad y_dt %d", y_dt);
  NVIT_REQUIRE(gate_args_ok(gate, rows_per_sample, M), "res_skip_bwd: with a gate, M=%d must be a multiple of rows_per_sample=%d", M,
               rows_per_sample);
  ResSkipArgs ar{dout, h, y, skip, x, dx, dh_lo, dh, part_dskip, M, C, gate, gate ? rows_per_sample : 1};
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * C * (20.0 + elem_bytes(y_dt) + (dh_lo ? elem_bytes(dt) : 0.0)) + gate_bytes(gate, M), s);
  const auto kernel = with_row_types(C, y_dt, dt, [&](auto nv, auto ty, auto tl) {
    return with_bool(gate != nullptr, [&](auto gated) { return &res_skip_bwd_kernel<nv, tag_t<decltype(ty)>, tag_t<decltype(tl)>, gated>; });
  });
  launch(kernel, dim3(nblk), dim3(256), 0, s, ar);
  NVIT_CHECK_LAUNCH("res_skip_bwd");
  return NVIT_OK;
}

// ---- head split / merge: compact heads (nvit_qknorm_*) and zero-padded ones (nvit_heads_pad_*, dp = PAD_D) ----
// Each entry point checks its own arguments and opens its ProfScope; these pick the instantiation and launch it (NORM when
// sqk is given).  dp: the stored head width (a.d: compact heads).
static void heads_split_launch(int dt, const QkArgs& a, int dp, hipStream_t s) {
  const bool norm = a.sqk != nullptr;
  const auto kernel = dp == a.d ? with_row_vecs<8>(a.H * a.d, [&](auto nv) {
    return with_bool(norm, [&](auto nm) {
      return with_in_out_elems(dt, [&](auto ti, auto to) {
        return &qknorm_fwd_kernel<nv, tag_t<decltype(ti)>, tag_t<decltype(to)>, nm>;
      });
    });
  }) : with_bool(norm, [&](auto nm) {
    return with_elem(dt, [&](auto to) { return &heads_pad_fwd_kernel<tag_t<decltype(to)>, nm>; });
  });
  launch(kernel, dim3(row_grid(a.B * a.T)), dim3(256), 0, s, a);
}

// with the normalise: nblk workgroups, one row of part each; the merge alone: a row grid (nblk unused)
static void heads_merge_launch(int dt, const QkBwdArgs& a, int dp, int nblk, hipStream_t s) {
  const bool norm = a.sqk != nullptr;
  const auto kernel = with_head_width(dp, [&](auto w) {
    return with_bool(norm, [&](auto nm) {
      return with_elem(dt, [&](auto t) { return &heads_merge_kernel<w, tag_t<decltype(t)>, nm>; });
    });
  });
  launch(kernel, dim3(norm ? nblk : row_grid(a.B * a.T)), dim3(256),
         norm ? (size_t)(ROW_WAVES + 2) * a.H * a.d * sizeof(float) : 0, s, a);
}

extern "C" int nvit_qknorm_fwd(int dt, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                               const float* sqk, float c_q, void* qh, void* kh, void* vh, float* rq, float* rk,
                               int B, int T, int H, int d, void* stream) {
  const int C = H * d;
  NVIT_REQUIRE(d == 16 || d == 32 || d == 64 || d == 128, "qknorm_fwd: head dim %d unsupported", d);
  NVIT_REQUIRE(C <= NVIT_MAX_EMBD && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0, "qknorm_fwd: bad C/ld");
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16 || dt == NVIT_BF16_F32IN, "qknorm_fwd: bad dt %d", dt);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)B * T * C * (dt == NVIT_F32 ? 24.0 : dt == NVIT_BF16 ? 12.0 : 18.0), s);
  heads_split_launch(dt, QkArgs{q, k, v, ldq, ldk, ldv, sqk, c_q, qh, kh, vh, rq, rk, nullptr, B, T, H, d}, d, s);
  NVIT_CHECK_LAUNCH("qknorm_fwd");
  return NVIT_OK;
}

extern "C" int nvit_qknorm_bwd(int dt, const void* dqh, const void* dkh, const void* dvh, const void* qh,
                               const void* kh, const float* rq, const float* rk, const float* sqk, float c_q,
                               void* dq, int ldq, void* dk, int ldk, void* dv, int ldv, float* part_dsqk, int nblk,
                               int B, int T, int H, int d, void* stream) {
  const int C = H * d;
  NVIT_REQUIRE(d == 16 || d == 32 || d == 64 || d == 128, "qknorm_bwd: head dim %d unsupported", d);
  NVIT_REQUIRE(C <= NVIT_MAX_EMBD && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0, "qknorm_bwd: bad C/ld");
  NVIT_REQUIRE(nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "qknorm_bwd: nblk out of range");
  // split without the normalise: the backward is the head merge alone (qh, kh, rq, rk, part unused)
  NVIT_REQUIRE(sqk || dt == NVIT_F32 || dt == NVIT_BF16, "qknorm_bwd: bad dt %d", dt);
  hipStream_t s = (hipStream_t)stream;
  const double eb = dt == NVIT_F32 ? 4.0 : 2.0;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)B * T * C * (sqk ? 8.0 : 6.0) * eb, s);
  heads_merge_launch(dt, QkBwdArgs{dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, dk, dv, ldq, ldk, ldv, part_dsqk, B, T, H, d},
                     d, nblk, s);
  NVIT_CHECK_LAUNCH("qknorm_bwd");
  return NVIT_OK;
}

static bool pad_dims_ok(int H, int d, int dp) {
  return dp == PAD_D && d > 0 && d < dp && d % 8 == 0 && H > 0 && H * d <= NVIT_MAX_EMBD;
}

extern "C" int nvit_heads_pad_fwd(int dt, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                  const float* sqk, float c_q, void* qh, void* kh, void* vh, float* rq, float* rk,
                                  float* sqk_pad, int B, int T, int H, int d, int dp, void* stream) {
  const int C = H * d;
  NVIT_REQUIRE(pad_dims_ok(H, d, dp), "heads_pad_fwd: needs dp = %d, head dim %d a multiple of 8 below dp, H*d <= %d", PAD_D, d, NVIT_MAX_EMBD);
  NVIT_REQUIRE(B > 0 && T > 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldq >= C && ldk >= C && ldv >= C,
               "heads_pad_fwd: bad shape/ld");
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16_F32IN, "heads_pad_fwd: dt %d (fp32 projections in: F32 or BF16_F32IN)", dt);
  NVIT_REQUIRE(q && k && v && qh && kh && vh && (!sqk || (rq && rk)), "heads_pad_fwd: missing pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)B * T * 3.0 * (C * 4.0 + H * dp * (dt == NVIT_F32 ? 4.0 : 2.0)), s);
  heads_split_launch(dt, QkArgs{q, k, v, ldq, ldk, ldv, sqk, c_q, qh, kh, vh, rq, rk, sqk_pad, B, T, H, d}, dp, s);
  NVIT_CHECK_LAUNCH("heads_pad_fwd");
  return NVIT_OK;
}

extern "C" int nvit_heads_pad_bwd(int dt, const void* dqh, const void* dkh, const void* dvh, const void* qh,
                                  const void* kh, const float* rq, const float* rk, const float* sqk, float c_q,
                                  void* dq, int ldq, void* dk, int ldk, void* dv, int ldv, float* part_dsqk, int nblk,
                                  int B, int T, int H, int d, int dp, void* stream) {
  const int C = H * d;
  NVIT_REQUIRE(pad_dims_ok(H, d, dp), "heads_pad_bwd: needs dp = %d, head dim %d a multiple of 8 below dp, H*d <= %d", PAD_D, d, NVIT_MAX_EMBD);
  NVIT_REQUIRE(B > 0 && T > 0 && ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldq >= C && ldk >= C && ldv >= C,
               "heads_pad_bwd: bad shape/ld");
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "heads_pad_bwd: bad dt %d", dt);
  NVIT_REQUIRE(dqh && dkh && dvh && dq && dk && dv, "heads_pad_bwd: missing pointer");
  if (sqk) {   // (the head merge alone uses no qh, kh, rq, rk, part_dsqk or nblk)
    NVIT_REQUIRE(qh && kh && rq && rk && part_dsqk, "heads_pad_bwd: missing pointer");
    NVIT_REQUIRE(nblk > 0 && nblk <= NVIT_MAX_PART_BLOCKS, "heads_pad_bwd: nblk out of range");
  }
  hipStream_t s = (hipStream_t)stream;
  const double eb = dt == NVIT_F32 ? 4.0 : 2.0;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)B * T * C * (sqk ? 8.0 : 6.0) * eb, s);
  heads_merge_launch(dt, QkBwdArgs{dqh, dkh, dvh, qh, kh, rq, rk, sqk, c_q, dq, dk, dv, ldq, ldk, ldv, part_dsqk, B, T, H, d},
                     dp, nblk, s);
  NVIT_CHECK_LAUNCH("heads_pad_bwd");
  return NVIT_OK;
}

static int pad_copy_grid(size_t groups) {
  const size_t blocks = (groups + 255) / 256;
  return (int)(blocks > 8192 ? 8192 : blocks);
}

extern "C" int nvit_pad_cols(int dt, const void* src, void* dst, int M, int H, int d, int dp, void* stream) {
  NVIT_REQUIRE(pad_dims_ok(H, d, dp) && M > 0 && src && dst, "pad_cols: needs dp = %d, head dim %d a multiple of 8 below dp, H*d <= %d", PAD_D, d, NVIT_MAX_EMBD);
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "pad_cols: bad dt %d", dt);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * H * (d + dp) * (dt == NVIT_F32 ? 4.0 : 2.0), s);
  with_elem(dt, [&](auto t) {
    using T = tag_t<decltype(t)>;
    launch(pad_cols_kernel<T>, dim3(pad_copy_grid((size_t)M * H * (dp / 4))), dim3(256), 0, s, (const T*)src, (T*)dst, M, H, d);
  });
  NVIT_CHECK_LAUNCH("pad_cols");
  return NVIT_OK;
}

extern "C" int nvit_unpad_cols(int dt, const void* src, void* dst, int M, int H, int d, int dp, void* stream) {
  NVIT_REQUIRE(pad_dims_ok(H, d, dp) && M > 0 && src && dst, "unpad_cols: needs dp = %d, head dim %d a multiple of 8 below dp, H*d <= %d", PAD_D, d, NVIT_MAX_EMBD);
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "unpad_cols: bad dt %d", dt);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * H * d * 2.0 * (dt == NVIT_F32 ? 4.0 : 2.0), s);
  with_elem(dt, [&](auto t) {
    using T = tag_t<decltype(t)>;
    launch(unpad_cols_kernel<T>, dim3(pad_copy_grid((size_t)M * H * d / 4)), dim3(256), 0, s, (const T*)src, (T*)dst, M, H, d);
  });
  NVIT_CHECK_LAUNCH("unpad_cols");
  return NVIT_OK;
}

static int swiglu_rows_per_blk(int M, int F) {
  const int colblocks = cdiv(F, 1024);
  int rowblocks = cdiv(2048, colblocks);
  int rpb = cdiv(M, rowblocks);
  return rpb < 1 ? 1 : rpb;
}

extern "C" int nvit_swiglu_fwd(int dt, const void* uv, const float* suv, float gscale, void* x, int M, int F,
                               void* stream) {
  NVIT_REQUIRE(F % 16 == 0 && M > 0, "swiglu_fwd: F=%d must be a multiple of 16", F);
  hipStream_t s = (hipStream_t)stream;
  const int rpb = swiglu_rows_per_blk(M, F);
  dim3 grid(cdiv(F, 1024), cdiv(M, rpb));
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16 || dt == NVIT_BF16_F32IN, "swiglu_fwd: bad dt %d", dt);
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * F * (dt == NVIT_F32 ? 12.0 : dt == NVIT_BF16 ? 6.0 : 10.0), s);
  // NVIT_BF16_F32IN: gated from the unrounded pre-activations (like the fused GEMM epilogue)
  with_in_out_elems(dt, [&](auto ti, auto to) {
    using TI = tag_t<decltype(ti)>;
    using T = tag_t<decltype(to)>;
    launch(swiglu_fwd_kernel<TI, T>, grid, dim3(256), 0, s, (const TI*)uv, suv, gscale, (T*)x, M, F, rpb);
  });
  NVIT_CHECK_LAUNCH("swiglu_fwd");
  return NVIT_OK;
}

extern "C" int nvit_swiglu_bwd(int dt, const void* dx, const void* uv, const float* suv, float gscale, void* duv,
                               float* part_dsuv, int rows_per_blk, int M, int F, void* stream) {
  NVIT_REQUIRE(F % 16 == 0 && M > 0 && rows_per_blk > 0, "swiglu_bwd: bad shape");
  NVIT_REQUIRE(!suv || part_dsuv, "swiglu_bwd: part_dsuv missing");
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(cdiv(F, 1024), cdiv(M, rows_per_blk));
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * F * 5.0 * (dt == NVIT_F32 ? 4 : 2), s);
  with_elem(dt, [&](auto t) {
    using T = tag_t<decltype(t)>;
    launch(swiglu_bwd_kernel<T>, grid, dim3(256), 0, s, (const T*)dx, (const T*)uv, suv, gscale, (T*)duv,
           suv ? part_dsuv : nullptr, M, F, rows_per_blk);
  });
  NVIT_CHECK_LAUNCH("swiglu_bwd");
  return NVIT_OK;
}

extern "C" int nvit_colsum_reduce(const float* part, int nblk, int N, float* out, int accumulate, int kind,
                                  const float* ref, float scale, void* stream) {
  NVIT_REQUIRE(kind == 0 || (kind == 1 && ref) || (kind == 2 && N % 32 == 0), "colsum_reduce: bad kind");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3(cdiv(N, 32)), dim3(1024), 0, s, part, nblk, N, out, accumulate, kind,
                     ref, scale);
  NVIT_CHECK_LAUNCH("colsum_reduce");
  return NVIT_OK;
}

// n <= 8 reductions in one launch.  Host arrays of n entries each; part_b[i] may be 0 (no second partial array).
extern "C" int nvit_colsum_reduce_multi(const int64_t* part, const int* nblk, const int64_t* part_b, const int* nblk_b,
                                        const int* N, const int64_t* out, const int* accumulate, const int* kind,
                                        const int64_t* ref, const float* scale, int n, void* stream) {
  NVIT_REQUIRE(n >= 1 && n <= CSR_MAX_ITEMS && part && nblk && part_b && nblk_b && N && out && accumulate && kind && ref && scale,
               "colsum_reduce_multi: 1..%d items", CSR_MAX_ITEMS);
  CsrBatch bt{};
  bt.n = n;
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    NVIT_REQUIRE(part[i] && out[i] && nblk[i] > 0 && N[i] > 0, "colsum_reduce_multi: item %d is empty", i);
    NVIT_REQUIRE(kind[i] == 0 || (kind[i] == 1 && ref[i]) || (kind[i] == 2 && N[i] % 32 == 0), "colsum_reduce_multi: bad kind");
    NVIT_REQUIRE(!part_b[i] || nblk_b[i] > 0, "colsum_reduce_multi: item %d: second partial array without rows", i);
    CsrItem& it = bt.it[i];
    it.part = reinterpret_cast<const float*>(part[i]);
    it.part_b = reinterpret_cast<const float*>(part_b[i]);
    it.ref = reinterpret_cast<const float*>(ref[i]);
    it.out = reinterpret_cast<float*>(out[i]);
    it.nblk = nblk[i];
    it.nblk_b = nblk_b[i];
    it.N = N[i];
    it.accumulate = accumulate[i];
    it.kind = kind[i];
    it.scale = scale[i];
    it.block0 = blocks;
    blocks += cdiv(N[i], 32);
  }
  hipLaunchKernelGGL(colsum_reduce_multi_kernel, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, bt);
  NVIT_CHECK_LAUNCH("colsum_reduce_multi");
  return NVIT_OK;
}

extern "C" int nvit_colsum(const void* a, int a_dt, int lda, const void* b, int b_dt, int ldb, int R, int N,
                           int period, float* out, int accumulate, float scale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int per = period > 0 ? period : 1;
  dim3 grid(cdiv(N, 128), per);
  with_elem(a_dt, [&](auto ta) {
    with_elem(b ? b_dt : NVIT_F32, [&](auto tb) {   // no b: the <TA, float> kernel
      using TA = tag_t<decltype(ta)>;
      using TB = tag_t<decltype(tb)>;
      launch(colsum_kernel<TA, TB>, grid, dim3(128), 0, s, (const TA*)a, lda, (const TB*)b, ldb, R, N, per, out, accumulate, scale);
    });
  });
  NVIT_CHECK_LAUNCH("colsum");
  return NVIT_OK;
}

extern "C" int nvit_cast(const float* src, void* dst, int dt, int64_t n, void* stream) {
  NVIT_REQUIRE(n % 4 == 0, "cast: n must be a multiple of 4");
  hipStream_t s = (hipStream_t)stream;
  const long long n4 = n / 4;
  int blocks = cdiv(n4, 256);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) return NVIT_OK;
  with_elem(dt, [&](auto t) {
    using T = tag_t<decltype(t)>;
    launch(cast_kernel<T>, dim3(blocks), dim3(256), 0, s, src, (T*)dst, n4);
  });
  NVIT_CHECK_LAUNCH("cast");
  return NVIT_OK;
}

extern "C" int nvit_normalize_images(const void* in, int in_is_u8_hwc, float* out, int B, int C, int H, int W, float mean,
                                     float std_, void* stream) {
  NVIT_REQUIRE(in && out && B > 0 && C > 0 && H > 0 && W > 0 && W % 4 == 0 && std_ != 0.f,
               "normalize_images: bad arguments (W must be a multiple of 4)");
  NVIT_REQUIRE(((uintptr_t)out & 15) == 0 && (in_is_u8_hwc || ((uintptr_t)in & 15) == 0),
               "normalize_images: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long n4 = (long long)B * C * H * (W / 4);
  int blocks = cdiv(n4, 256);
  if (blocks > 8192) blocks = 8192;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)n4 * 4.0 * (in_is_u8_hwc ? 5.0 : 8.0), s);
  if (in_is_u8_hwc)
    hipLaunchKernelGGL(normalize_images_kernel<unsigned char>, dim3(blocks), dim3(256), 0, s, (const unsigned char*)in, out,
                       B, C, H, W, mean, 1.0f / std_);
  else
    hipLaunchKernelGGL(normalize_images_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)in, out, B, C, H, W,
                       mean, 1.0f / std_);
  NVIT_CHECK_LAUNCH("normalize_images");
  return NVIT_OK;
}

extern "C" int nvit_scale_cols(const float* a, int lda, const float* sc, float c, void* out, int out_dt, int ldo,
                               int R, int N, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(cdiv(N, 128), R);
  with_elem(out_dt, [&](auto t) {
    using T = tag_t<decltype(t)>;
    launch(scale_cols_kernel<T>, grid, dim3(128), 0, s, a, lda, sc, c, (T*)out, ldo, R, N);
  });
  NVIT_CHECK_LAUNCH("scale_cols");
  return NVIT_OK;
}
