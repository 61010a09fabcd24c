// impl 0: scalar-FMA attention kernels (any element type, fp32 math).  They carry the exact-f32
// parity mode and serve as the on-device cross-check of the MFMA flash kernels (attn_mfma.hip).
// S lanes own one query (fwd, dq) or one key (dk/dv); the other side is streamed through
// LDS in tiles of 32 rows and read by broadcast.
#include "attn_mfma.h"
#include "dispatch.h"

namespace {

constexpr int TILE = 32;

// Lanes per query (or key).  One lane per row up to head dim 64.  At 128 one thread would need q[128] + acc[128] live
// registers, more than the architectural file holds, so S = 4 adjacent lanes share a row, lane j owning the channels
// e = S*i + j (i < D / S; the S lanes of a row read S consecutive words of an LDS row: no bank conflict).  Dot products are
// the lane partials summed by a butterfly over the S lanes (every lane ends with the same bits); at S = 1 that is the plain
// sum over e in order.
constexpr int lanes_per_row(int D) { return D > 64 ? 4 : 1; }

template <int S>
__device__ __forceinline__ float split_sum(float v) {
#pragma unroll
  for (int o = 1; o < S; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Fills two [TILE][D] LDS tiles as fp32 from rows row_a.. of a and row_b.. of b (row strides lda, ldb elements); rows from
// n on are zero.  The caller puts the barriers around it.
template <typename T, int D>
__device__ __forceinline__ void stage_tiles(float (&as)[TILE][D], float (&bs)[TILE][D], const T* a, size_t row_a, int lda,
                                            const T* b, size_t row_b, int ldb, int n) {
  for (int i = threadIdx.x; i < TILE * D; i += 64) {
    const int r = i / D, e = i % D;
    float av = 0.f, bv = 0.f;
    if (r < n) {   // one branch, both loads in flight before the first LDS store
      av = (float)a[(row_a + r) * lda + e];
      bv = (float)b[(row_b + r) * ldb + e];
    }
    as[r][e] = av;
    bs[r][e] = bv;
  }
}

template <typename T, int D, int S>
__global__ __launch_bounds__(64) void attn_fwd_ref(const T* qh, const T* kh, const T* vh, float scale, T* o,
                                                    float* lse, int H, int Tq, int Tk) {
  constexpr int DL = D / S;
  __shared__ float ks[TILE][D], vs[TILE][D];
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int j = threadIdx.x % S;
  const int qi = blockIdx.x * (64 / S) + threadIdx.x / S;
  const bool ok = qi < Tq;
  const T* qp = qh + ((size_t)bh * Tq + (ok ? qi : 0)) * D;
  float q[DL], acc[DL];
#pragma unroll
  for (int i = 0; i < DL; ++i) {
    q[i] = (float)qp[S * i + j] * scale;
    acc[i] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < Tk; k0 += TILE) {
    const int nk = min(TILE, Tk - k0);
    stage_tiles<T, D>(ks, vs, kh, (size_t)bh * Tk + k0, D, vh, (size_t)bh * Tk + k0, D, nk);
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < DL; ++i) s += q[i] * ks[kk][S * i + j];
      s = split_sum<S>(s);
      const float mn = fmaxf(m, s);
      const float corr = expf(m - mn), p = expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int i = 0; i < DL; ++i) acc[i] = acc[i] * corr + p * vs[kk][S * i + j];
      m = mn;
    }
    __syncthreads();
  }
  if (ok) {
    const float inv = 1.0f / l;
    T* op = o + ((size_t)b * Tq + qi) * (H * D) + h * D;
#pragma unroll
    for (int i = 0; i < DL; ++i) op[S * i + j] = (T)(acc[i] * inv);
    if (j == 0) lse[(size_t)bh * Tq + qi] = m + logf(l);
  }
}

// delta[b,h,t] = sum_e dO[b,t,h*D+e] * O[b,t,h*D+e].  One thread per 8 consecutive channels of a
// token row (coalesced 16/32-byte loads); the D/8 lanes of a head are adjacent and reduce by shuffles.
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(const T* dout, const T* o, float* delta, int B, int H,
                                                          int Tq, int D) {
  const int C8 = (H * D) >> 3, G = D >> 3;  // chunks per row, lanes per head (4 or 8)
  const long long total = (long long)B * Tq * C8;
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  float s = 0.f;
  long long m = 0;
  int c8 = 0;
  if (idx < total) {
    m = idx / C8;
    c8 = (int)(idx % C8);
    const size_t off = (size_t)m * (H * D) + (size_t)c8 * 8;
    const f32x4 a0 = load4<T>(dout + off), a1 = load4<T>(dout + off + 4);
    const f32x4 b0 = load4<T>(o + off), b1 = load4<T>(o + off + 4);
    s = a0[0] * b0[0] + a0[1] * b0[1] + a0[2] * b0[2] + a0[3] * b0[3] + a1[0] * b1[0] + a1[1] * b1[1] +
        a1[2] * b1[2] + a1[3] * b1[3];
  }
  s = group_sum_dyn(s, G);
  if (idx < total && (c8 % G) == 0) {
    const int h = c8 / G;
    const int b = (int)(m / Tq), t = (int)(m % Tq);
    delta[((size_t)b * H + h) * Tq + t] = s;
  }
}

template <typename T, int D, int S>
__global__ __launch_bounds__(64) void attn_bwd_dq_ref(const T* dout, const T* qh, const T* kh, const T* vh,
                                                       const float* lse, const float* delta, float scale, T* dqh,
                                                       int H, int Tq, int Tk) {
  constexpr int DL = D / S;
  __shared__ float ks[TILE][D], vs[TILE][D];
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int j = threadIdx.x % S;
  const int qi = blockIdx.x * (64 / S) + threadIdx.x / S;
  const bool ok = qi < Tq;
  const int qc = ok ? qi : 0;
  const T* qp = qh + ((size_t)bh * Tq + qc) * D;
  const T* gp = dout + ((size_t)b * Tq + qc) * (H * D) + h * D;
  float q[DL], g[DL], acc[DL];
#pragma unroll
  for (int i = 0; i < DL; ++i) {
    q[i] = (float)qp[S * i + j] * scale;
    g[i] = (float)gp[S * i + j];
    acc[i] = 0.f;
  }
  const float L = lse[(size_t)bh * Tq + qc], dl = delta[(size_t)bh * Tq + qc];
  for (int k0 = 0; k0 < Tk; k0 += TILE) {
    const int nk = min(TILE, Tk - k0);
    stage_tiles<T, D>(ks, vs, kh, (size_t)bh * Tk + k0, D, vh, (size_t)bh * Tk + k0, D, nk);
    __syncthreads();
    for (int kk = 0; kk < nk; ++kk) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int i = 0; i < DL; ++i) {
        s += q[i] * ks[kk][S * i + j];
        dp += g[i] * vs[kk][S * i + j];
      }
      s = split_sum<S>(s);
      dp = split_sum<S>(dp);
      const float p = expf(s - L);
      const float ds = p * (dp - dl) * scale;
#pragma unroll
      for (int i = 0; i < DL; ++i) acc[i] += ds * ks[kk][S * i + j];
    }
    __syncthreads();
  }
  if (ok) {
    T* op = dqh + ((size_t)bh * Tq + qi) * D;
#pragma unroll
    for (int i = 0; i < DL; ++i) op[S * i + j] = (T)acc[i];
  }
}

template <typename T, int D, int S>
__global__ __launch_bounds__(64) void attn_bwd_dkv_ref(const T* dout, const T* qh, const T* kh, const T* vh,
                                                        const float* lse, const float* delta, float scale, T* dkh,
                                                        T* dvh, int H, int Tq, int Tk) {
  constexpr int DL = D / S;
  __shared__ float qs[TILE][D], gs[TILE][D];
  __shared__ float ls[TILE], ds_[TILE];
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int j = threadIdx.x % S;
  const int ki = blockIdx.x * (64 / S) + threadIdx.x / S;
  const bool ok = ki < Tk;
  const int kc = ok ? ki : 0;
  float k[DL], v[DL], dk[DL], dv[DL];
#pragma unroll
  for (int i = 0; i < DL; ++i) {
    k[i] = (float)kh[((size_t)bh * Tk + kc) * D + S * i + j];
    v[i] = (float)vh[((size_t)bh * Tk + kc) * D + S * i + j];
    dk[i] = 0.f;
    dv[i] = 0.f;
  }
  for (int q0 = 0; q0 < Tq; q0 += TILE) {
    const int nq = min(TILE, Tq - q0);
    stage_tiles<T, D>(qs, gs, qh, (size_t)bh * Tq + q0, D, dout + h * D, (size_t)b * Tq + q0, H * D, nq);
    if (threadIdx.x < TILE) {
      const bool in = threadIdx.x < nq;
      ls[threadIdx.x] = in ? lse[(size_t)bh * Tq + q0 + threadIdx.x] : 0.f;
      ds_[threadIdx.x] = in ? delta[(size_t)bh * Tq + q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    for (int qq = 0; qq < nq; ++qq) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int i = 0; i < DL; ++i) {
        s += qs[qq][S * i + j] * k[i];
        dp += gs[qq][S * i + j] * v[i];
      }
      s = split_sum<S>(s);
      dp = split_sum<S>(dp);
      const float p = expf(s * scale - ls[qq]);
      const float dsv = p * (dp - ds_[qq]) * scale;
#pragma unroll
      for (int i = 0; i < DL; ++i) {
        dv[i] += p * gs[qq][S * i + j];
        dk[i] += dsv * qs[qq][S * i + j];
      }
    }
    __syncthreads();
  }
  if (ok) {
#pragma unroll
    for (int i = 0; i < DL; ++i) {
      dkh[((size_t)bh * Tk + ki) * D + S * i + j] = (T)dk[i];
      dvh[((size_t)bh * Tk + ki) * D + S * i + j] = (T)dv[i];
    }
  }
}

}  // namespace

static int attn_fwd_impl(int dt, int impl, const void* qh, const void* kh, const void* vh, float scale, const float* sqk,
                         float c_q, float qpre, void* o, float* lse, int B, int H, int Tq, int Tk, int d, void* stream);

extern "C" int nvit_attn_fwd(int dt, int impl, const void* qh, const void* kh, const void* vh, float scale, void* o,
                             float* lse, int B, int H, int Tq, int Tk, int d, void* stream) {
  return attn_fwd_impl(dt, impl, qh, kh, vh, scale, nullptr, 0.f, 1.0f, o, lse, B, H, Tq, Tk, d, stream);
}

// nViT call sites: q and k are (sqk*c_q) * unit vectors per head, which bounds every score; the MFMA kernel then skips
// the running maximum (see attn_mfma.hip).  Same result as nvit_attn_fwd up to rounding.  q_prescale: qh holds
// q_prescale * q_hat (the producer folded the factor into the learned scale); 1 = plain.  With q_prescale =
// scale * log2(e) the MFMA kernel's exponent needs no multiply (the fused training path).
// sqk == NULL: no bound (plain-ViT heads from the split-only q/k/v epilogue): the running-maximum kernel, q pre-scaled.
extern "C" int nvit_attn_fwd_bounded(int dt, int impl, const void* qh, const void* kh, const void* vh, float scale,
                                     const float* sqk, float c_q, float q_prescale, void* o, float* lse, int B, int H,
                                     int Tq, int Tk, int d, void* stream) {
  NVIT_REQUIRE(q_prescale > 0.f, "attn_fwd_bounded: q_prescale must be positive");
  return attn_fwd_impl(dt, impl, qh, kh, vh, scale, sqk, c_q, q_prescale, o, lse, B, H, Tq, Tk, d, stream);
}

static int attn_fwd_impl(int dt, int impl, const void* qh, const void* kh, const void* vh, float scale, const float* sqk,
                         float c_q, float qpre, void* o, float* lse, int B, int H, int Tq, int Tk, int d, void* stream) {
  NVIT_REQUIRE(d == 32 || d == 64 || d == 128, "attn_fwd: head dim %d unsupported (32, 64 or 128)", d);
  NVIT_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "attn_fwd: empty problem");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ATTN_FWD, 4.0 * B * H * (double)Tq * Tk * d, 0.0, s);
  if (impl == 1) {
    NVIT_REQUIRE(dt == NVIT_BF16, "attn_fwd: MFMA kernel needs bf16");
    return nvit_attn_fwd_mfma(qh, kh, vh, scale, qpre, sqk, c_q, o, lse, B, H, Tq, Tk, d, s);
  }
  scale = scale / qpre;   // the scalar kernels take the multiplier of q.k directly
  with_elem(dt, [&](auto t) {
    with_head_dim(d, [&](auto hd) {
      using T = tag_t<decltype(t)>;
      constexpr int S = lanes_per_row(hd);
      launch(attn_fwd_ref<T, hd, S>, dim3(cdiv(Tq, 64 / S), B * H), dim3(64), 0, s, (const T*)qh, (const T*)kh,
             (const T*)vh, scale, (T*)o, lse, H, Tq, Tk);
    });
  });
  NVIT_CHECK_LAUNCH("attn_fwd_ref");
  return NVIT_OK;
}

extern "C" int nvit_attn_bwd(int dt, int impl, const void* dout, const void* qh, const void* kh, const void* vh,
                             const void* o, const float* lse, float scale, void* dqh, void* dkh, void* dvh,
                             float* delta, int B, int H, int Tq, int Tk, int d, void* stream) {
  NVIT_REQUIRE(d == 32 || d == 64 || d == 128, "attn_bwd: head dim %d unsupported (32, 64 or 128)", d);
  NVIT_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "attn_bwd: empty problem");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ATTN_BWD, 10.0 * B * H * (double)Tq * Tk * d, 0.0, s);
  if (impl == 1) {
    // the MFMA dq kernel computes delta = rowsum(dO * O) itself and leaves it in `delta` for the dk/dv kernel
    NVIT_REQUIRE(dt == NVIT_BF16, "attn_bwd: MFMA kernel needs bf16");
    return nvit_attn_bwd_mfma(dout, qh, kh, vh, o, lse, delta, scale, dqh, dkh, dvh, B, H, Tq, Tk, d, s);
  }
  const long long total = (long long)B * Tq * ((H * d) / 8);
  with_elem(dt, [&](auto t) {
    using T = tag_t<decltype(t)>;
    launch(attn_delta_kernel<T>, dim3(cdiv(total, 256)), dim3(256), 0, s, (const T*)dout, (const T*)o, delta, B, H, Tq, d);
  });
  NVIT_CHECK_LAUNCH("attn_delta");
  with_elem(dt, [&](auto t) {
    with_head_dim(d, [&](auto hd) {
      using T = tag_t<decltype(t)>;
      constexpr int S = lanes_per_row(hd);
      launch(attn_bwd_dq_ref<T, hd, S>, dim3(cdiv(Tq, 64 / S), B * H), dim3(64), 0, s, (const T*)dout, (const T*)qh,
             (const T*)kh, (const T*)vh, lse, delta, scale, (T*)dqh, H, Tq, Tk);
      launch(attn_bwd_dkv_ref<T, hd, S>, dim3(cdiv(Tk, 64 / S), B * H), dim3(64), 0, s, (const T*)dout, (const T*)qh,
             (const T*)kh, (const T*)vh, lse, delta, scale, (T*)dkh, (T*)dvh, H, Tq, Tk);
    });
  });
  NVIT_CHECK_LAUNCH("attn_bwd_ref");
  return NVIT_OK;
}

// MFMA attention backward (bf16, d = 64) with the q/k-normalise backward fused into the epilogues; with sqk == NULL (and
// rq, rk, part_q, part_k unused) the epilogues store dq / dk / dv token-major as they are (plain-ViT heads).
extern "C" int nvit_attn_bwd_qknorm(int dt, const void* dout, const void* qh, const void* kh, const void* vh,
                                    const void* o, const float* lse, float scale, const float* rq, const float* rk,
                                    const float* sqk, float c_q, float q_prescale, void* dq, int ldq, void* dk, void* dv,
                                    int ldkv, float* part_q, float* part_k, float* delta, int B, int H, int Tq, int Tk,
                                    int d, void* stream) {
  NVIT_REQUIRE(dt == NVIT_BF16 && d == 64, "attn_bwd_qknorm: needs bf16 and head dim 64");
  NVIT_REQUIRE(B > 0 && H > 0 && Tq > 0 && Tk > 0, "attn_bwd_qknorm: empty problem");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_ATTN_BWD, 10.0 * B * H * (double)Tq * Tk * d, 0.0, s);
  return nvit_attn_bwd_mfma_fused(dout, qh, kh, vh, o, lse, delta, scale, rq, rk, sqk, c_q, q_prescale, dq, ldq, dk, dv,
                                  ldkv, part_q, part_k, B, H, Tq, Tk, d, s);
}
