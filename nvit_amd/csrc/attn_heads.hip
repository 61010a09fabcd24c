// Head-axis attention: what the reference's flash_attn=True branch computes (model.py:121-122, 252-253).
// flash_attn_func reads its [B,H,T,d] arguments as [batch, seqlen, nheads, headdim], so its softmax runs over the H heads
// of one token:  out[m, i, :] = sum_j softmax_j(scale * <q~[m,i,:], k~[m,j,:]>) v[m,j,:],  i, j < H.
// No token mixing: per token this is H x H scores over d, i.e. 4*H*C FLOP against 16*C bytes moved - a streaming row
// kernel, not an MFMA one.
//
// Mapping (both directions): one wave owns one token (grid-strided rows, one-wave workgroups so the per-token LDS stage
// scales with C and not with a fixed wave count).  Lane l owns columns c = (i*64 + l)*4 .. +3 of slot i < NV, i.e. the
// four elements r = c % D .. +3 of head h = c / D; the D/4 lanes of one head form an aligned group inside a slot.  The
// rows every lane must see for every head (k~ and v forward; q~ and dO in the second backward phase) are staged in LDS;
// a score <q~_h, k~_j> is four FMAs per lane plus a log2(D/4)-step group reduction, and every group of the wave computes
// its own query head's score against key head j at once, so a token costs H (not H^2) reduction rounds per slot.
//
// q, k, v are read as fp32 (the unrounded projection GEMM outputs, as the unfused SDPA route reads them): the normalise
// runs on the unrounded values and bf16 appears only in what is stored (O, dq, dk, dv).
#include "dispatch.h"

namespace {

struct HeadsArgs {
  const float *q, *k, *v;
  int ldq, ldkv;
  const float* sqk;  // [C], NULL: plain heads (no normalise)
  float c_q, scale;
  const void* dout;  // backward: dO [M, C], type T
  void* o;           // forward: O [M, C], type T
  float* lse;        // [M, H] natural-log softmax denominators (forward writes, backward reads)
  void *dq, *dk, *dv;
  int lddq, lddkv;
  float* part;       // backward: [gridDim.x, C] partial sums of d/d(sqk*c_q)
  int M, H;
};

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

template <int NV, int D, typename T, bool NORM>
__global__ __launch_bounds__(64) void attn_heads_fwd_kernel(HeadsArgs a) {
  extern __shared__ f32x4 lds4[];
  float* ks = reinterpret_cast<float*>(lds4);  // k~ [C]
  const int H = a.H, C = H * D;
  float* vs = ks + C;                          // v  [C]
  constexpr int G = D / 4;
  const int lane = threadIdx.x;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 s[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    s[i] = (NORM && c < C) ? load4<float>(a.sqk + c) * a.c_q : z;
  }
  for (int m = blockIdx.x; m < a.M; m += gridDim.x) {
    f32x4 qn[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const bool ok = c < C;
      f32x4 q4 = ok ? load4<float>(a.q + (size_t)m * a.ldq + c) : z;
      f32x4 k4 = ok ? load4<float>(a.k + (size_t)m * a.ldkv + c) : z;
      const f32x4 v4 = ok ? load4<float>(a.v + (size_t)m * a.ldkv + c) : z;
      if constexpr (NORM) {
        const float sq = group_sum<G>(dot4(q4, q4)), sk = group_sum<G>(dot4(k4, k4));
        const float rq = ok ? 1.0f / sqrtf(sq) : 0.f, rk = ok ? 1.0f / sqrtf(sk) : 0.f;
        q4 = q4 * rq * s[i];
        k4 = k4 * rk * s[i];
      }
      qn[i] = q4;
      if (ok) {
        *reinterpret_cast<f32x4*>(ks + c) = k4;
        *reinterpret_cast<f32x4*>(vs + c) = v4;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const bool ok = c < C;
      const int r = c % D;
      float mx = -INFINITY, l = 0.f;
      f32x4 acc = z;
      for (int j = 0; j < H; ++j) {
        const f32x4 kk = ok ? *reinterpret_cast<const f32x4*>(ks + j * D + r) : z;
        const f32x4 vv = ok ? *reinterpret_cast<const f32x4*>(vs + j * D + r) : z;
        const float sc = group_sum<G>(dot4(qn[i], kk)) * a.scale;
        const float mn = fmaxf(mx, sc);
        const float corr = expf(mx - mn), p = expf(sc - mn);
        l = l * corr + p;
        acc = acc * corr + vv * p;
        mx = mn;
      }
      if (ok) {
        store4<T>(reinterpret_cast<T*>(a.o) + (size_t)m * C + c, acc * (1.0f / l));
        if (r == 0) a.lse[(size_t)m * H + c / D] = mx + logf(l);
      }
    }
    __syncthreads();  // the next token overwrites the stage
  }
}

// Backward, per token: (1) k~, v and the inverse norms staged; (2) lanes as query heads i: P_ij recomputed from the saved
// lse, dP_ij = <dO_i, v_j>, D_i = sum_j P_ij dP_ij, dS_ij = P_ij (dP_ij - D_i), dq~_i = scale * sum_j dS_ij k~_j, then the
// normalise backward of q; (3) q~ and dO staged over k~, v; lanes as key heads j: dv_j = sum_i P_ij dO_i,
// dk~_j = scale * sum_i dS_ij q~_i, then the normalise backward of k.  The d(sqk*c_q) column partials gather
// dq~ * n_q + dk~ * n_k over the block's tokens in registers, in a fixed order (no atomics).
template <int NV, int D, typename T, bool NORM>
__global__ __launch_bounds__(64) void attn_heads_bwd_kernel(HeadsArgs a) {
  extern __shared__ f32x4 lds4[];
  const int H = a.H, C = H * D;
  float* X = reinterpret_cast<float*>(lds4);  // k~, then q~  [C]
  float* Y = X + C;                            // v,  then dO  [C]
  float* P = Y + C;                            // [H, H] probabilities (row = query head)
  float* DP = P + H * H;                       // [H, H] dP
  float* DS = DP + H * H;                      // [H, H] dS
  float* rn = DS + H * H;                      // [2H] 1/||q_h||, 1/||k_h||
  constexpr int G = D / 4;
  const int lane = threadIdx.x;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 s[NV], ds[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    s[i] = (NORM && c < C) ? load4<float>(a.sqk + c) * a.c_q : z;
    ds[i] = z;
  }
  for (int m = blockIdx.x; m < a.M; m += gridDim.x) {
    const float* qrow = a.q + (size_t)m * a.ldq;
    const float* krow = a.k + (size_t)m * a.ldkv;
    const T* dorow = reinterpret_cast<const T*>(a.dout) + (size_t)m * C;
    // (1) stage k~, v; inverse norms
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const bool ok = c < C;
      f32x4 k4 = ok ? load4<float>(krow + c) : z;
      const f32x4 v4 = ok ? load4<float>(a.v + (size_t)m * a.ldkv + c) : z;
      if constexpr (NORM) {
        const f32x4 q4 = ok ? load4<float>(qrow + c) : z;
        const float sq = group_sum<G>(dot4(q4, q4)), sk = group_sum<G>(dot4(k4, k4));
        const float rq = ok ? 1.0f / sqrtf(sq) : 0.f, rk = ok ? 1.0f / sqrtf(sk) : 0.f;
        k4 = k4 * rk * s[i];
        if (ok && c % D == 0) {
          rn[c / D] = rq;
          rn[H + c / D] = rk;
        }
      }
      if (ok) {
        *reinterpret_cast<f32x4*>(X + c) = k4;
        *reinterpret_cast<f32x4*>(Y + c) = v4;
      }
    }
    __syncthreads();
    // (2) lanes as query heads
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const bool ok = c < C;
      const int r = c % D, h = ok ? c / D : 0;
      f32x4 q4 = ok ? load4<float>(qrow + c) : z;
      float rq = 0.f;
      if constexpr (NORM) {
        rq = rn[h];
        q4 = q4 * rq;  // unit vector n_q
      }
      const f32x4 qt = NORM ? q4 * s[i] : q4;
      const f32x4 do4 = ok ? load4<T>(dorow + c) : z;
      const float lse = ok ? a.lse[(size_t)m * H + h] : 0.f;
      float Di = 0.f;
      for (int j = 0; j < H; ++j) {
        const f32x4 kk = ok ? *reinterpret_cast<const f32x4*>(X + j * D + r) : z;
        const f32x4 vv = ok ? *reinterpret_cast<const f32x4*>(Y + j * D + r) : z;
        const float sc = group_sum<G>(dot4(qt, kk));
        const float dp = group_sum<G>(dot4(do4, vv));
        const float p = expf(sc * a.scale - lse);
        Di += p * dp;
        if (ok && r == 0) {
          P[h * H + j] = p;
          DP[h * H + j] = dp;
        }
      }
      __syncthreads();
      f32x4 g = z;
      for (int j = 0; j < H; ++j) {
        const float dsv = ok ? P[h * H + j] * (DP[h * H + j] - Di) : 0.f;
        const f32x4 kk = ok ? *reinterpret_cast<const f32x4*>(X + j * D + r) : z;
        g += kk * dsv;
        if (ok && r == 0) DS[h * H + j] = dsv;
      }
      g = g * a.scale;  // d/d q~
      if constexpr (NORM) {
        ds[i] += g * q4;
        const f32x4 sg = g * s[i];
        const float dn = group_sum<G>(dot4(sg, q4));
        g = (sg - q4 * dn) * rq;
      }
      if (ok) store4<T>(reinterpret_cast<T*>(a.dq) + (size_t)m * a.lddq + c, g);
    }
    __syncthreads();
    // (3) stage q~ and dO over k~ and v; lanes as key heads
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < C) {
        f32x4 q4 = load4<float>(qrow + c);
        if constexpr (NORM) q4 = q4 * rn[c / D] * s[i];
        *reinterpret_cast<f32x4*>(X + c) = q4;
        *reinterpret_cast<f32x4*>(Y + c) = load4<T>(dorow + c);
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      const bool ok = c < C;
      const int r = c % D, h = ok ? c / D : 0;
      f32x4 gk = z, gv = z;
      for (int ii = 0; ii < H; ++ii) {
        const f32x4 qq = ok ? *reinterpret_cast<const f32x4*>(X + ii * D + r) : z;
        const f32x4 dd = ok ? *reinterpret_cast<const f32x4*>(Y + ii * D + r) : z;
        const float p = ok ? P[ii * H + h] : 0.f, dsv = ok ? DS[ii * H + h] : 0.f;
        gv += dd * p;
        gk += qq * dsv;
      }
      gk = gk * a.scale;  // d/d k~
      if constexpr (NORM) {
        const float rk = ok ? rn[H + h] : 0.f;
        const f32x4 nk = (ok ? load4<float>(krow + c) : z) * rk;
        ds[i] += gk * nk;
        const f32x4 sg = gk * s[i];
        const float dn = group_sum<G>(dot4(sg, nk));
        gk = (sg - nk * dn) * rk;
      }
      if (ok) {
        store4<T>(reinterpret_cast<T*>(a.dk) + (size_t)m * a.lddkv + c, gk);
        store4<T>(reinterpret_cast<T*>(a.dv) + (size_t)m * a.lddkv + c, gv);
      }
    }
    __syncthreads();  // the next token overwrites the stage
  }
  if constexpr (NORM) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < C) *reinterpret_cast<f32x4*>(a.part + (size_t)blockIdx.x * C + c) = ds[i];
    }
  }
}

}  // namespace

// (NV, D, T, NORM) of a call: rows up to 16 vectors per lane, the head dim, the element type of o / dout and the
// gradients, and whether q and k are normalised here (sqk given)
template <typename F>
static auto with_heads_types(int C, int d, int dt, bool norm, F&& f) {
  return with_row_vecs<16>(C, [&](auto nv) {
    return with_head_dim(d, [&](auto hd) {
      return with_elem(dt, [&](auto t) { return with_bool(norm, [&](auto nm) { return f(nv, hd, t, nm); }); });
    });
  });
}

static int heads_check(int dt, int M, int H, int d, int ldq, int ldkv) {
  NVIT_REQUIRE(dt == NVIT_F32 || dt == NVIT_BF16, "attn_heads: bad dt %d", dt);
  NVIT_REQUIRE(d == 32 || d == 64 || d == 128, "attn_heads: head dim %d unsupported (32, 64, 128)", d);
  NVIT_REQUIRE(H >= 1 && H <= NVIT_ATTN_HEADS_MAX_H, "attn_heads: %d heads, at most %d are built", H,
               NVIT_ATTN_HEADS_MAX_H);
  NVIT_REQUIRE(M >= 0 && ldq % 4 == 0 && ldkv % 4 == 0 && ldq >= H * d && ldkv >= H * d, "attn_heads: bad M/ld");
  return NVIT_OK;
}

extern "C" int nvit_attn_heads_fwd(int dt, const float* q, int ldq, const float* k, const float* v, int ldkv,
                                   const float* sqk, float c_q, float scale, void* o, float* lse, int M, int H, int d,
                                   void* stream) {
  const int rc = heads_check(dt, M, H, d, ldq, ldkv);
  if (rc != NVIT_OK) return rc;
  if (M == 0) return NVIT_OK;
  const int C = H * d;
  HeadsArgs a{q, k, v, ldq, ldkv, sqk, c_q, scale, nullptr, o, lse, nullptr, nullptr, nullptr, 0, 0, nullptr, M, H};
  hipStream_t s = (hipStream_t)stream;
  const int ncu = nvit_num_cu();
  const int cap = 32 * (ncu > 0 ? ncu : 256);
  const int grid = M < cap ? M : cap;
  const size_t shm = (size_t)2 * C * sizeof(float);
  const double esz = dt == NVIT_F32 ? 4.0 : 2.0;
  ProfScope ps(NVIT_KID_ATTN_FWD, 4.0 * M * H * C, (double)M * C * (12.0 + esz) + 4.0 * M * H, s);
  const auto kernel = with_heads_types(C, d, dt, sqk != nullptr, [](auto nv, auto hd, auto t, auto nm) {
    return &attn_heads_fwd_kernel<nv, hd, tag_t<decltype(t)>, nm>;
  });
  launch(kernel, dim3(grid), dim3(64), shm, s, a);
  NVIT_CHECK_LAUNCH("attn_heads_fwd");
  return NVIT_OK;
}

extern "C" int nvit_attn_heads_bwd(int dt, const void* dout, const float* q, int ldq, const float* k, const float* v,
                                   int ldkv, const float* sqk, float c_q, float scale, const float* lse, void* dq,
                                   int lddq, void* dk, void* dv, int lddkv, float* part_dsqk, int nblk, int M, int H,
                                   int d, void* stream) {
  const int rc = heads_check(dt, M, H, d, ldq, ldkv);
  if (rc != NVIT_OK) return rc;
  const int C = H * d;
  NVIT_REQUIRE(lddq >= C && lddkv >= C && lddq % 4 == 0 && lddkv % 4 == 0, "attn_heads_bwd: bad output ld");
  NVIT_REQUIRE(nblk > 0 && nblk <= NVIT_ATTN_HEADS_BWD_MAX_BLOCKS, "attn_heads_bwd: nblk %d out of range", nblk);
  NVIT_REQUIRE(!sqk || part_dsqk, "attn_heads_bwd: part_dsqk is required with sqk");
  HeadsArgs a{q, k, v, ldq, ldkv, sqk, c_q, scale, dout, nullptr, const_cast<float*>(lse), dq, dk, dv, lddq, lddkv,
              part_dsqk, M, H};
  hipStream_t s = (hipStream_t)stream;
  const size_t shm = ((size_t)2 * C + 3 * H * H + 2 * H) * sizeof(float);
  const double esz = dt == NVIT_F32 ? 4.0 : 2.0;
  ProfScope ps(NVIT_KID_ATTN_BWD, 8.0 * M * H * C, (double)M * C * (12.0 + 4.0 * esz) + 4.0 * M * H, s);
  const auto kernel = with_heads_types(C, d, dt, sqk != nullptr, [](auto nv, auto hd, auto t, auto nm) {
    return &attn_heads_bwd_kernel<nv, hd, tag_t<decltype(t)>, nm>;
  });
  launch(kernel, dim3(nblk), dim3(64), shm, s, a);
  NVIT_CHECK_LAUNCH("attn_heads_bwd");
  return NVIT_OK;
}
