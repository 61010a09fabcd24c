// On-device AutoAugment input pipeline: uint8 [B,H,W,C] batch in, the model's fp32 [B,C,H,W] input
// out, in two launches that a hipGraph can capture.
//
//   nvit_augment_draw   one workgroup: Philox4x32-10 per image -> int32 [B,2,8] parameter table (op id + 7 arguments);
//                       the step counter is a device int64 that the kernel itself advances.
//   nvit_augment_apply  one workgroup per image: the two ops in sequence, then ToTensor + Normalize with exactly
//                       nvit_normalize_images' arithmetic.
//
// The ops are Pillow's (the AutoAugment paper's released code), restated in integers and contraction-free fp32/fp64 so
// that the result is bit-identical to Pillow's: tests/augment_ref.py is the numpy twin, tests/golden/augment_pil.npz the
// Pillow fixture.  Everything that depends on the whole image goes through one mechanism: a per-channel 256-bin
// histogram in LDS (gray mean of Contrast, min/max of AutoContrast, the cumulative table of Equalize), from which a
// 256-entry per-channel lookup table is built; the pointwise ops build the same table without the histogram.  Only the
// affine ops, Color (needs the pixel's three channels) and Sharpness (3x3 stencil) read the image directly.
// An op reads one complete image and writes another: the intermediate images live in a caller-provided global workspace
// (two per image, each used by this workgroup only, so they stay in L2), which makes one code path for every image size.
//
// RandAugment (timm's rand-m9-mstd0.5-inc1 family; tests/randaug_ref.py is the numpy twin) stands in AutoAugment's place:
//   nvit_randaug_draw   one workgroup: one Philox call per (image, layer) -> int32 [B,L,16] table; op, on / off, a
//                       continuous magnitude, sign and filter; the level maps in fp64
//   nvit_randaug_apply  one workgroup per image: the L ops in sequence, then the same ToTensor + Normalize.  The
//                       geometric ops are Pillow's ImagingGenericTransform, fp64 bilinear / bicubic with a fill colour;
//                       the others are apply_op's, plus SolarizeAdd as one more lookup table.
//
// Further down, the batch-level mixing that follows it (Mixup / CutMix, tests/mix_ref.py is the numpy twin), here for the
// file-wide contract(off) (the Philox function is philox.h's, shared with crop.hip):
//   nvit_mix_draw       one workgroup, one thread per pair of rows -> int32 [B,8] table, lambda and the partner's label
//   nvit_mix_apply      fp32 [B,C,H,W] -> fp32 [B,C,H,W], float4 streaming over (pair, chunk of the image)
// and the one draw that sits inside the model, stochastic depth (tests/droppath_ref.py is the numpy twin):
//   nvit_droppath_draw  one workgroup -> fp32 [2*n_layer, B] gates of the gated row kernels (rowops.hip)
#include "common.h"
#include "philox.h"

// a fused a + f*b changes truncations by one level: nothing in this file contracts, except normalize4 below.  (Plain
// operators on purpose: the __fmul_rn/__fadd_rn of the HIP headers are inline a*b / a+b compiled under the headers' own
// default contraction, and the compiler does fuse a pair of them.)
#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 1024;
constexpr int AUG_HIST_COPIES = 4;   // waves spread over four histogram copies: a low-contrast image hits few bins
constexpr int AUG_ROW = NVIT_AUG_ROW;           // ints per op in the parameter table
constexpr int AUG_NOPS = NVIT_AUG_NOPS;
constexpr int AUG_NMAG = NVIT_AUG_NMAG;

enum AugOp { OP_IDENTITY = 0, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR,
             OP_CONTRAST, OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT,
             OP_SOLARIZE_ADD = NVIT_RA_SOLARIZE_ADD /* RandAugment only: nvit_augment_apply knows ids below AUG_NOPS */ };
static_assert(OP_INVERT + 1 == AUG_NOPS && OP_SOLARIZE_ADD == AUG_NOPS && NVIT_RA_NOPS == OP_SOLARIZE_ADD + 1, "op ids");

// policy: int32 [P,2,3] = (op, probability as fp32 bits, magnitude index); argtab: int32 [15,10,2,8], the parameter row
// of every (op, magnitude index, sign) for this image size, computed by the host in fp64.
__global__ __launch_bounds__(256) void augment_draw_kernel(const int* __restrict__ policy, int P,
                                                           unsigned long long seed, long long* step_ctr,
                                                           long long first_index, const int* __restrict__ argtab,
                                                           int* __restrict__ params, int B) {
  const unsigned long long step = (unsigned long long)*step_ctr;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const unsigned long long g = (unsigned long long)(first_index + i);
    const Philox4 r = philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)(step >> 32),
                                    (unsigned)seed, (unsigned)(seed >> 32));
    const int sub = (int)(((unsigned long long)r.v[0] * (unsigned long long)P) >> 32);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int* e = policy + (sub * 2 + k) * 3;
      const float u = (float)(r.v[1 + k] >> 8) * 0x1p-24f;   // exact: 24 bits
      const bool on = u < __int_as_float(e[1]);
      const int sign = (r.v[3] >> k) & 1;
      const int* src = argtab + ((e[0] * AUG_NMAG + e[2]) * 2 + sign) * AUG_ROW;
      int* dst = params + ((size_t)i * 2 + k) * AUG_ROW;
#pragma unroll
      for (int j = 0; j < AUG_ROW; ++j) dst[j] = on ? src[j] : 0;   // off: Identity
    }
  }
  __syncthreads();   // every thread has read the counter
  if (threadIdx.x == 0) *step_ctr = (long long)(step + 1);
}

// ------------------------------------------------------------------------------------------------ the ops
__device__ __forceinline__ int gray_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (uint8) clamp(deg + f * (x - deg), 0, 255): fp32, multiply then add, truncating (Pillow's ImagingBlend)
__device__ __forceinline__ unsigned char blend(int deg, int x, float f) {
  const float t = (float)deg + f * (float)(x - deg);   // two roundings (file-wide contract(off))
  return (unsigned char)(t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t));
}

struct AugShared {
  unsigned hist[AUG_HIST_COPIES][3][256];
  unsigned char lut[3][256];
  int lo[3], hi[3];
  int mean;
};

// Per-channel histograms of src into sh.hist[0] (channel 0 holds the gray histogram when `of_gray`).
__device__ void histogram(AugShared& sh, const unsigned char* src, int N, int C, bool of_gray) {
  unsigned* h = &sh.hist[0][0][0];
  for (int i = threadIdx.x; i < AUG_HIST_COPIES * 3 * 256; i += AUG_THREADS) h[i] = 0;
  __syncthreads();
  unsigned(*mine)[256] = sh.hist[(threadIdx.x >> 6) & (AUG_HIST_COPIES - 1)];
  if (of_gray) {
    for (int p = threadIdx.x; p < N; p += AUG_THREADS) {
      const unsigned char* q = src + (size_t)p * C;
      atomicAdd(&mine[0][C == 3 ? gray_of(q[0], q[1], q[2]) : q[0]], 1u);
    }
  } else {
    for (int i = threadIdx.x; i < N * C; i += AUG_THREADS) atomicAdd(&mine[i % C][src[i]], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 256; i += AUG_THREADS) {
    unsigned s = h[i];
#pragma unroll
    for (int k = 1; k < AUG_HIST_COPIES; ++k) s += h[k * 3 * 256 + i];
    h[i] = s;
  }
  __syncthreads();
}

// One op: src (complete image, uint8 HWC) -> dst.  id and a[] are uniform over the workgroup.
__device__ void apply_op(AugShared& sh, const unsigned char* src, unsigned char* dst, int id, const int* a, int H, int W,
                         int C) {
  const int N = H * W;
  const int tid = threadIdx.x;
  if (id >= OP_SHEAR_X && id <= OP_ROTATE) {
    // Pillow's affine_fixed: 16.16 output-to-input coefficients, nearest, fill 0
    const int a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
    for (int p = tid; p < N; p += AUG_THREADS) {
      const int y = p / W, x = p - y * W;
      const int xin = (a2 + a1 * y + a0 * x) >> 16, yin = (a5 + a4 * y + a3 * x) >> 16;
      const bool ok = xin >= 0 && xin < W && yin >= 0 && yin < H;
      const unsigned char* q = src + (ok ? (size_t)yin * W + xin : (size_t)0) * C;   // always inside the image
      for (int c = 0; c < C; ++c) dst[(size_t)p * C + c] = ok ? q[c] : (unsigned char)0;
    }
    return;
  }
  const float f = __int_as_float(a[0]);
  if (id == OP_COLOR) {
    for (int p = tid; p < N; p += AUG_THREADS) {
      const unsigned char* q = src + (size_t)p * C;
      if (C == 3) {
        const int r = q[0], g = q[1], b = q[2], gr = gray_of(r, g, b);
        dst[(size_t)p * 3 + 0] = blend(gr, r, f);
        dst[(size_t)p * 3 + 1] = blend(gr, g, f);
        dst[(size_t)p * 3 + 2] = blend(gr, b, f);
      } else {
        dst[p] = q[0];   // the gray of a one-channel image is the channel itself
      }
    }
    return;
  }
  if (id == OP_SHARPNESS) {
    // Pillow's SMOOTH: (1,1,1,1,5,1,1,1,1)/13 rounded, border pixels unchanged
    for (int i = tid; i < N * C; i += AUG_THREADS) {
      const int p = i / C, c = i - p * C;
      const int y = p / W, x = p - y * W;
      const int v = src[i];
      int deg = v;
      if (y > 0 && y < H - 1 && x > 0 && x < W - 1) {
        int acc = 4 * v;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) acc += src[((size_t)(y + dy) * W + (x + dx)) * C + c];
        deg = (2 * acc + 13) / 26;
      }
      dst[i] = blend(deg, v, f);
    }
    return;
  }
  // ---- the rest is a per-channel lookup table
  if (id == OP_CONTRAST || id == OP_AUTOCONTRAST || id == OP_EQUALIZE) {
    histogram(sh, src, N, C, id == OP_CONTRAST);
    if (id == OP_CONTRAST) {
      if (tid == 0) {
        unsigned long long s = 0;
        for (int i = 0; i < 256; ++i) s += (unsigned long long)i * sh.hist[0][0][i];
        sh.mean = (int)((2 * s + (unsigned long long)N) / (2ull * N));
      }
    } else if (tid < C) {
      const unsigned* h = sh.hist[0][tid];
      int lo = 256, hi = -1;
      for (int i = 0; i < 256; ++i)
        if (h[i]) {
          if (lo == 256) lo = i;
          hi = i;
        }
      sh.lo[tid] = lo;
      sh.hi[tid] = hi;
      if (id == OP_EQUALIZE) {
        // Pillow's ImageOps.equalize: step from the histogram without its last occupied bin
        const unsigned step = ((unsigned)N - h[hi]) / 255u;
        unsigned n = step / 2;
        for (int i = 0; i < 256; ++i) {
          unsigned v = i;
          if (step != 0 && hi > lo) {
            v = n / step;
            v = v > 255u ? 255u : v;
          }
          sh.lut[tid][i] = (unsigned char)v;
          n += h[i];
        }
      }
    }
    __syncthreads();
  }
  if (id != OP_EQUALIZE) {
    for (int t = tid; t < C * 256; t += AUG_THREADS) {
      const int c = t >> 8, i = t & 255;
      int v = i;
      switch (id) {
        case OP_BRIGHTNESS: v = blend(0, i, f); break;
        case OP_CONTRAST: v = blend(sh.mean, i, f); break;
        case OP_POSTERIZE: v = i & ~(0xFF >> a[0]); break;
        case OP_SOLARIZE: v = i >= a[0] ? 255 - i : i; break;
        case OP_INVERT: v = 255 - i; break;
        case OP_SOLARIZE_ADD: v = i < 128 ? (i + a[0] > 255 ? 255 : i + a[0]) : i; break;
        case OP_AUTOCONTRAST: {
          const int lo = sh.lo[c], hi = sh.hi[c];
          if (hi > lo) {
            // Pillow computes this table in Python floats (fp64)
            const double scale = 255.0 / (double)(hi - lo);
            const double off = (double)-lo * scale;
            const double d = (double)i * scale + off;
            v = d <= 0.0 ? 0 : (d >= 255.0 ? 255 : (int)d);
          }
          break;
        }
        default: break;
      }
      sh.lut[c][i] = (unsigned char)v;
    }
  }
  __syncthreads();
  for (int i = tid; i < N * C; i += AUG_THREADS) dst[i] = sh.lut[i % C][src[i]];
}

// ToTensor + Normalize of four pixels, written as nvit_normalize_images writes it (rowops.hip) and compiled, like it,
// under the compiler's default contraction, so that the two give the same bits.
__device__ __forceinline__ f32x4 normalize4(const unsigned char* p, int C, float mean, float inv_std) {
#pragma clang fp contract(fast)
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (float)p[(size_t)e * C] * (1.0f / 255.0f);
  return (v - mean) * inv_std;
}

// The end of both apply kernels: image b's augmented uint8 [H,W,C] and / or its fp32 [C,H,W], ToTensor + Normalize.
__device__ __forceinline__ void write_outputs(const unsigned char* cur, float* out_f32, unsigned char* out_u8, int b, int H,
                                              int W, int C, float mean, float inv_std) {
  const size_t n = (size_t)H * W * C;
  if (out_u8) {
    unsigned char* o = out_u8 + (size_t)b * n;
    for (size_t i = threadIdx.x; i < n; i += AUG_THREADS) o[i] = cur[i];
  }
  if (out_f32) {
    const int w4 = W / 4, n4 = C * H * w4;
    for (int i = threadIdx.x; i < n4; i += AUG_THREADS) {
      const int x4 = (i % w4) * 4;
      int r = i / w4;
      const int y = r % H, c = r / H;
      *reinterpret_cast<f32x4*>(out_f32 + (((size_t)b * C + c) * H + y) * W + x4) =
          normalize4(cur + ((size_t)y * W + x4) * C + c, C, mean, inv_std);
    }
  }
}

__global__ __launch_bounds__(AUG_THREADS) void augment_apply_kernel(const unsigned char* in,
                                                                    const int* __restrict__ params, float* out_f32,
                                                                    unsigned char* out_u8, unsigned char* ws,
                                                                    size_t ws_stride, int B, int H, int W, int C, float mean,
                                                                    float inv_std) {
  __shared__ AugShared sh;
  const int b = blockIdx.x;
  const size_t n = (size_t)H * W * C;
  const unsigned char* cur = in + (size_t)b * n;
  unsigned char* buf[2] = {ws + (size_t)(2 * b) * ws_stride, ws + (size_t)(2 * b + 1) * ws_stride};
  for (int k = 0; k < 2; ++k) {
    const int* row = params + ((size_t)b * 2 + k) * AUG_ROW;
    const int id = row[0];
    if (id <= OP_IDENTITY || id >= AUG_NOPS) continue;   // Identity; ids come from the host's tables, which know no others
    apply_op(sh, cur, buf[k], id, row + 1, H, W, C);
    cur = buf[k];
    __syncthreads();   // the op's stores are visible to the workgroup before the next pass reads them
  }
  write_outputs(cur, out_f32, out_u8, b, H, W, C, mean, inv_std);
}

// ------------------------------------------------------------------------------------------------ RandAugment
// (tests/randaug_ref.py is the numpy twin and fixes which Philox word feeds which decision.)
constexpr int RA_ROW = NVIT_RA_ROW;             // id, filter, six fp64 coefficients or one int argument, padding
constexpr int RA_KNOTS = NVIT_RA_ROT_KNOTS;
constexpr unsigned RA_DOMAIN = 0x52414E44u;     // + layer, xor-ed into the key's high word
// timm's _RAND_INCREASING_TRANSFORMS, in its order: the op index of the draw -> op id
__constant__ int RA_CHOICES[NVIT_RA_NCHOICES] = {OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_ROTATE, OP_POSTERIZE,
                                                 OP_SOLARIZE, OP_SOLARIZE_ADD, OP_COLOR, OP_CONTRAST, OP_BRIGHTNESS,
                                                 OP_SHARPNESS, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y};

// q: fp64 [NVIT_ERASE_KNOTS + 1] normal quantiles; rot: fp64 [2, RA_KNOTS + 1], cos then sin at k / rot_scale degrees.
__global__ __launch_bounds__(256) void randaug_draw_kernel(unsigned long long seed, long long* step_ctr, long long first_index,
                                                           const double* __restrict__ q, const double* __restrict__ rot,
                                                           double magnitude, double mstd, int mstd_inf, double mmax,
                                                           int increasing, float prob, int interp, double translate_pct,
                                                           double rot_scale, int* __restrict__ params, int B, int L, int H,
                                                           int W) {
  const unsigned long long step = (unsigned long long)*step_ctr;
  for (int t = threadIdx.x; t < B * L; t += blockDim.x) {
    const int i = t / L, layer = t - i * L;
    const unsigned long long g = (unsigned long long)(first_index + i);
    const Philox4 r = philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)(step >> 32),
                                    (unsigned)seed, (unsigned)(seed >> 32) ^ (RA_DOMAIN + (unsigned)layer));
    const int id = RA_CHOICES[(int)(((unsigned long long)r.v[0] * (unsigned long long)NVIT_RA_NCHOICES) >> 32)];
    const bool on = (float)(r.v[1] >> 8) * 0x1p-24f < prob;   // exact: 24 bits
    const unsigned u = r.v[2] >> 8;
    double m = magnitude;
    if (mstd_inf) {
      m = magnitude * ((double)u * 0x1p-24);   // timm's uniform(0, magnitude)
    } else if (mstd > 0.0) {
      const int kn = (int)(u >> 14);
      const double f = (double)(u & 0x3FFFu) * 0x1p-14;
      m = magnitude + mstd * (q[kn] + f * (q[kn + 1] - q[kn]));
    }
    m = m > mmax ? mmax : m;
    m = m < 0.0 ? 0.0 : m;
    const double lv = m / 10.0;
    const bool neg = (r.v[3] & 1u) != 0;
    const int filter = interp == NVIT_RA_RANDOM ? (int)((r.v[3] >> 1) & 1u) : interp;

    int* row = params + (size_t)t * RA_ROW;
    double* coef = reinterpret_cast<double*>(row + 2);   // 8-byte aligned: the row is 64 bytes
    if (!on) {
#pragma unroll
      for (int j = 0; j < RA_ROW; ++j) row[j] = 0;
      continue;
    }
    row[0] = id;
    row[14] = 0;
    row[15] = 0;
    if (id >= OP_SHEAR_X && id <= OP_ROTATE) {
      row[1] = filter;
      double a0 = 1.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 1.0, a5 = 0.0;
      if (id == OP_ROTATE) {
        // Image.rotate's matrix about (W/2, H/2) at -/+ 30 lv degrees, cos / sin from the host's table
        const double pos = (lv * 30.0) * rot_scale;
        int kn = (int)pos;
        kn = kn > RA_KNOTS - 1 ? RA_KNOTS - 1 : kn;
        const double f = pos - (double)kn;
        const double c = rot[kn] + f * (rot[kn + 1] - rot[kn]);
        const double sa = rot[RA_KNOTS + 1 + kn] + f * (rot[RA_KNOTS + 2 + kn] - rot[RA_KNOTS + 1 + kn]);
        const double s = neg ? sa : -sa;   // r = -radians(deg), deg = -angle when negated
        const double cx = (double)W / 2.0, cy = (double)H / 2.0;
        a0 = c;
        a1 = s;
        a2 = c * -cx + s * -cy + 0.0 + cx;
        a3 = -s;
        a4 = c;
        a5 = -s * -cx + c * -cy + 0.0 + cy;
      } else if (id == OP_SHEAR_X || id == OP_SHEAR_Y) {
        const double v = lv * 0.3;
        (id == OP_SHEAR_X ? a1 : a3) = neg ? -v : v;
      } else {
        const double v = lv * translate_pct;   // relative: a fraction of the side, not rounded to pixels
        if (id == OP_TRANSLATE_X) {
          a2 = (neg ? -v : v) * (double)W;
        } else {
          a5 = (neg ? -v : v) * (double)H;
        }
      }
      coef[0] = a0;
      coef[1] = a1;
      coef[2] = a2;
      coef[3] = a3;
      coef[4] = a4;
      coef[5] = a5;
      continue;
    }
    int arg = 0;
    if (id >= OP_BRIGHTNESS && id <= OP_SHARPNESS) {
      double f;
      if (increasing) {
        const double v = lv * 0.9;
        f = 1.0 + (neg ? -v : v);
        f = f < 0.1 ? 0.1 : f;
      } else {
        f = lv * 1.8 + 0.1;
      }
      arg = __float_as_int((float)f);
    } else if (id == OP_POSTERIZE) {
      const int bits = (int)(lv * 4.0);
      arg = increasing ? 4 - bits : bits;
    } else if (id == OP_SOLARIZE) {
      int th = (int)(lv * 256.0);
      th = th > 256 ? 256 : th;
      arg = increasing ? 256 - th : th;
    } else if (id == OP_SOLARIZE_ADD) {
      arg = (int)(lv * 110.0);
      arg = arg > 128 ? 128 : arg;
    }
    row[1] = 0;
    row[2] = arg;
#pragma unroll
    for (int j = 3; j < 14; ++j) row[j] = 0;
  }
  __syncthreads();   // every thread has read the counter
  if (threadIdx.x == 0) *step_ctr = (long long)(step + 1);
}

__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2, p2 = -v1 + v3, p3 = 2.0 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// Pillow's ImagingGenericTransform with affine_transform and the bilinear / bicubic filter of 8-bit images, in fp64 and
// operation for operation (nothing here contracts).  Every index is clamped into the image, whatever the coefficients.
__device__ void affine_f64(const unsigned char* src, unsigned char* dst, const double* __restrict__ a, bool bicubic, int H,
                           int W, int C, int fill0, int fill1, int fill2) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
  const int N = H * W;
  for (int p = threadIdx.x; p < N; p += AUG_THREADS) {
    const int y = p / W, x = p - y * W;
    const double xi = (double)x + 0.5, yi = (double)y + 0.5;
    double xin = a0 * xi + a1 * yi + a2, yin = a3 * xi + a4 * yi + a5;
    unsigned char* o = dst + (size_t)p * C;
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {   // (also a NaN from a hand-written table)
      o[0] = (unsigned char)fill0;
      if (C == 3) {
        o[1] = (unsigned char)fill1;
        o[2] = (unsigned char)fill2;
      }
      continue;
    }
    xin = xin - 0.5;
    yin = yin - 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const int x0 = (int)fx, y0 = (int)fy;   // -1 .. W-1, -1 .. H-1
    const double dx = xin - fx, dy = yin - fy;
    if (!bicubic) {
      const int xl = clampi(x0, 0, W - 1), xr = clampi(x0 + 1, 0, W - 1);
      const unsigned char* r1 = src + (size_t)clampi(y0, 0, H - 1) * W * C;
      const bool has2 = y0 + 1 >= 0 && y0 + 1 < H;
      const unsigned char* r2 = src + (size_t)clampi(y0 + 1, 0, H - 1) * W * C;
      for (int c = 0; c < C; ++c) {
        const double p0 = (double)r1[xl * C + c], p1 = (double)r1[xr * C + c];
        const double v1 = p0 + (p1 - p0) * dx;
        double v2 = v1;
        if (has2) {
          const double q0 = (double)r2[xl * C + c], q1 = (double)r2[xr * C + c];
          v2 = q0 + (q1 - q0) * dx;
        }
        const double v = v1 + (v2 - v1) * dy;
        o[c] = (unsigned char)(v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v));   // (0 <= v <= 255 already: truncation)
      }
    } else {
      int xs[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[k] = clampi(x0 - 1 + k, 0, W - 1) * C;
      for (int c = 0; c < C; ++c) {
        // row y0-1 clamped; each of y0, y0+1, y0+2 if inside the image, otherwise the row before it again
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int yy = y0 - 1 + k;
          if (k == 0 || (yy >= 0 && yy < H)) {
            const unsigned char* r = src + (size_t)clampi(yy, 0, H - 1) * W * C + c;
            v[k] = cubic((double)r[xs[0]], (double)r[xs[1]], (double)r[xs[2]], (double)r[xs[3]], dx);
          } else {
            v[k] = v[k - 1];
          }
        }
        const double t = cubic(v[0], v[1], v[2], v[3], dy);
        o[c] = (unsigned char)(t <= 0.0 ? 0 : (t >= 255.0 ? 255 : (int)t));
      }
    }
  }
}

__global__ __launch_bounds__(AUG_THREADS) void randaug_apply_kernel(const unsigned char* in, const int* __restrict__ params,
                                                                    float* out_f32, unsigned char* out_u8, unsigned char* ws,
                                                                    size_t ws_stride, int B, int H, int W, int C, int L,
                                                                    int fill0, int fill1, int fill2, float mean,
                                                                    float inv_std) {
  __shared__ AugShared sh;
  const int b = blockIdx.x;
  const size_t n = (size_t)H * W * C;
  const unsigned char* cur = in + (size_t)b * n;
  unsigned char* buf[2] = {ws + (size_t)(2 * b) * ws_stride, ws + (size_t)(2 * b + 1) * ws_stride};
  int next = 0;   // the buffer that does not hold `cur`: a layer that is off must not make an op write what it reads
  for (int k = 0; k < L; ++k) {
    const int* row = params + ((size_t)b * L + k) * RA_ROW;
    const int id = row[0];
    if (id <= OP_IDENTITY || id >= NVIT_RA_NOPS) continue;   // layer off
    if (id >= OP_SHEAR_X && id <= OP_ROTATE) {
      affine_f64(cur, buf[next], reinterpret_cast<const double*>(row + 2), row[1] == NVIT_RA_BICUBIC, H, W, C, fill0, fill1,
                 fill2);
    } else {
      int arg = row[2];   // integer arguments of a hand-written table stay in their ranges (a factor is any float)
      if (id == OP_POSTERIZE) arg = clampi(arg, 0, 8);
      if (id == OP_SOLARIZE) arg = clampi(arg, 0, 256);
      if (id == OP_SOLARIZE_ADD) arg = clampi(arg, 0, 255);
      apply_op(sh, cur, buf[next], id, &arg, H, W, C);
    }
    cur = buf[next];
    next ^= 1;
    __syncthreads();   // the op's stores are visible to the workgroup before the next pass reads them
  }
  write_outputs(cur, out_f32, out_u8, b, H, W, C, mean, inv_std);
}

// ------------------------------------------------------------------------------------------------ Mixup / CutMix
// (tests/mix_ref.py is the numpy twin.)  Rows i and B-1-i of the batch form pair i.
constexpr int MIX_ROW = NVIT_MIX_ROW;                  // mode, lambda bits, y0, y1, x0, x1, partner row, 0
constexpr unsigned MIX_DOMAIN = 0x4D495821u;   // xor-ed into the key's high word: not AutoAugment's stream
constexpr int MIX_KNOTS = NVIT_MIX_KNOTS;             // the quantile tables hold MIX_KNOTS + 1 floats
enum MixMode { MIX_NONE = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2 };


// q_mix / q_cut: the Beta(alpha, alpha) quantile at k/MIX_KNOTS, k = 0..MIX_KNOTS, of the mode's alpha; NULL = mode off.
__global__ __launch_bounds__(256) void mix_draw_kernel(unsigned long long seed, long long* step_ctr, long long first_index,
                                                       const float* __restrict__ q_mix, const float* __restrict__ q_cut,
                                                       float prob, float switch_prob, const int64_t* __restrict__ labels,
                                                       int* __restrict__ table, float* __restrict__ lam_out,
                                                       int64_t* __restrict__ y2, int B, int H, int W) {
  const unsigned long long step = (unsigned long long)*step_ctr;
  const int npairs = (B + 1) / 2;
  for (int p = threadIdx.x; p < npairs; p += blockDim.x) {
    const int i = p, j = B - 1 - p;
    const unsigned long long g = (unsigned long long)(first_index + p);
    const Philox4 r = philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)(step >> 32),
                                    (unsigned)seed, (unsigned)(seed >> 32) ^ MIX_DOMAIN);
    const bool gate = (float)(r.v[0] >> 8) * 0x1p-24f < prob;   // exact: 24 bits
    const bool sw = (float)(r.v[1] >> 8) * 0x1p-24f < switch_prob;
    const bool cut = q_cut && (!q_mix || sw);
    const float* q = cut ? q_cut : q_mix;
    int mode = MIX_NONE, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    float lam = 1.0f;
    if (gate && q && i != j) {
      const unsigned u = r.v[2] >> 8;
      const int k = (int)(u >> 14);                           // 0..1023
      const float f = (float)(u & 0x3FFFu) * 0x1p-14f;        // exact
      lam = q[k] + f * (q[k + 1] - q[k]);                     // three roundings (file-wide contract(off))
      mode = MIX_MIXUP;
      if (cut) {
        // timm's rand_bbox with correct_lam, in fp64
        const int cy = (int)(((r.v[3] & 0xFFFFu) * (unsigned)H) >> 16), cx = (int)(((r.v[3] >> 16) * (unsigned)W) >> 16);
        const double ratio = __dsqrt_rn((double)(1.0f - lam));
        const int cut_h = (int)((double)H * ratio), cut_w = (int)((double)W * ratio);
        y0 = clampi(cy - cut_h / 2, 0, H);
        y1 = clampi(cy + cut_h / 2, 0, H);
        x0 = clampi(cx - cut_w / 2, 0, W);
        x1 = clampi(cx + cut_w / 2, 0, W);
        lam = (float)(1.0 - (double)((y1 - y0) * (x1 - x0)) / (double)(H * W));
        mode = MIX_CUTMIX;
      }
    }
    const int64_t yi = labels[i], yj = labels[j];
    for (int s = 0; s < (i == j ? 1 : 2); ++s) {
      const int b = s ? j : i;
      int* row = table + (size_t)b * MIX_ROW;
      row[0] = mode;
      row[1] = __float_as_int(lam);
      row[2] = y0;
      row[3] = y1;
      row[4] = x0;
      row[5] = x1;
      row[6] = s ? i : j;
      row[7] = 0;
      lam_out[b] = lam;
      y2[b] = s ? yi : yj;
    }
  }
  __syncthreads();   // every thread has read the counter
  if (threadIdx.x == 0) *step_ctr = (long long)(step + 1);
}

constexpr int MIX_THREADS = 256;
constexpr int MIX_PER_THREAD = 4;   // float4s of each of the two images per thread: 8 independent 16-byte loads in flight

// Grid (chunks of an image, rows).  The workgroups of row b serve the pair (b, partner) when b is its lower row and
// return at once when b is the upper one; a row that is not mixed (mode 0, its own partner, or a table whose partner
// does not name it back) is copied, or left alone in place.  Every element is read and written by one thread, so
// out == in is allowed.
__global__ __launch_bounds__(MIX_THREADS) void mix_apply_kernel(const float* in, const int* __restrict__ table, float* out,
                                                                int B, int n4, int H, int w4) {
  const int b = blockIdx.y;
  const int* row = table + (size_t)b * MIX_ROW;
  const int mode = row[0], j = row[6];
  const bool paired = (mode == MIX_MIXUP || mode == MIX_CUTMIX) && j >= 0 && j < B && j != b &&
                      table[(size_t)j * MIX_ROW + 6] == b && table[(size_t)j * MIX_ROW] == mode;
  const int base = blockIdx.x * (MIX_THREADS * MIX_PER_THREAD) + threadIdx.x;
  const size_t img = (size_t)n4 * 4;
  if (!paired) {
    if (in == out) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(in + (size_t)b * img);
    f32x4* dst = reinterpret_cast<f32x4*>(out + (size_t)b * img);
#pragma unroll
    for (int k = 0; k < MIX_PER_THREAD; ++k) {
      const int i = base + k * MIX_THREADS;
      if (i < n4) dst[i] = src[i];
    }
    return;
  }
  if (j < b) return;   // the lower row's workgroups write both images
  const f32x4* a_in = reinterpret_cast<const f32x4*>(in + (size_t)b * img);
  const f32x4* b_in = reinterpret_cast<const f32x4*>(in + (size_t)j * img);
  f32x4* a_out = reinterpret_cast<f32x4*>(out + (size_t)b * img);
  f32x4* b_out = reinterpret_cast<f32x4*>(out + (size_t)j * img);
  f32x4 va[MIX_PER_THREAD], vb[MIX_PER_THREAD];
#pragma unroll
  for (int k = 0; k < MIX_PER_THREAD; ++k) {
    const int i = base + k * MIX_THREADS;
    if (i < n4) {
      va[k] = a_in[i];
      vb[k] = b_in[i];
    }
  }
  if (mode == MIX_MIXUP) {
    const float lam = __int_as_float(row[1]), om = 1.0f - lam;
#pragma unroll
    for (int k = 0; k < MIX_PER_THREAD; ++k) {
      const int i = base + k * MIX_THREADS;
      if (i < n4) {
        a_out[i] = lam * va[k] + om * vb[k];   // two rounded products and one add (file-wide contract(off))
        b_out[i] = lam * vb[k] + om * va[k];
      }
    }
  } else {
    const int y0 = row[2], y1 = row[3], x0 = row[4], x1 = row[5];
#pragma unroll
    for (int k = 0; k < MIX_PER_THREAD; ++k) {
      const int i = base + k * MIX_THREADS;
      if (i < n4) {
        const int x = (i % w4) * 4, y = (i / w4) % H;
        const bool in_rows = y >= y0 && y < y1;
        f32x4 oa, ob;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool inside = in_rows && x + e >= x0 && x + e < x1;
          oa[e] = inside ? vb[k][e] : va[k][e];
          ob[e] = inside ? va[k][e] : vb[k][e];
        }
        a_out[i] = oa;
        b_out[i] = ob;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stochastic depth
// (tests/droppath_ref.py is the numpy twin.)  table fp32 [2*n_layer, B]: row 2*l + br holds the gates of
// branch br (0 attention, 1 MLP) of block l for every sample.  One Philox call per gate: the counter is (first_index + b,
// step) as in the other draws, the row index is added to the domain constant in the key's high word (the 128-bit
// counter is full), so a sample's gate depends on its global index, the step and the row only.
constexpr unsigned DROPPATH_DOMAIN = 0x44525054u;

__global__ __launch_bounds__(256) void droppath_draw_kernel(unsigned long long seed, long long* step_ctr, long long first_index,
                                                            const float* __restrict__ rates, int scale_by_keep,
                                                            float* __restrict__ table, int n_layer, int B) {
  const unsigned long long step = (unsigned long long)*step_ctr;
  const int n = 2 * n_layer * B;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int row = i / B, b = i - row * B;
    const unsigned long long g = (unsigned long long)(first_index + b);
    const Philox4 r = philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)(step >> 32),
                                    (unsigned)seed, (unsigned)(seed >> 32) ^ (DROPPATH_DOMAIN + (unsigned)row));
    const float keep = 1.0f - rates[row >> 1];
    const bool kept = (float)(r.v[0] >> 8) * 0x1p-24f < keep;   // exact: 24 bits
    table[i] = kept ? (scale_by_keep ? 1.0f / keep : 1.0f) : 0.0f;
  }
  __syncthreads();   // every thread has read the counter
  if (threadIdx.x == 0) *step_ctr = (long long)(step + 1);
}

}  // namespace

extern "C" int nvit_droppath_draw(uint64_t seed, int64_t* step, int64_t first_index, const float* rates, int scale_by_keep,
                                  float* table, int n_layer, int B, void* stream) {
  NVIT_REQUIRE(step && rates && table && first_index >= 0, "droppath_draw: bad arguments");
  NVIT_REQUIRE(n_layer > 0 && B > 0 && (long long)n_layer * B <= NVIT_DROPPATH_MAX_GATES / 2,
               "droppath_draw: 2 * n_layer * B must be in 1..%d", NVIT_DROPPATH_MAX_GATES);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, 2.0 * n_layer * B * 4.0, s);
  hipLaunchKernelGGL(droppath_draw_kernel, dim3(1), dim3(256), 0, s, (unsigned long long)seed, (long long*)step,
                     (long long)first_index, rates, scale_by_keep, table, n_layer, B);
  NVIT_CHECK_LAUNCH("droppath_draw");
  return NVIT_OK;
}

extern "C" int nvit_mix_draw(uint64_t seed, int64_t* step, int64_t first_index, const float* q_mix, const float* q_cut,
                             float prob, float switch_prob, const int64_t* labels, int* table, float* lam, int64_t* y2,
                             int B, int H, int W, void* stream) {
  NVIT_REQUIRE(step && labels && table && lam && y2 && B > 0 && first_index >= 0, "mix_draw: bad arguments");
  NVIT_REQUIRE(H > 0 && W > 0 && H <= NVIT_AUG_MAX_SIDE && W <= NVIT_AUG_MAX_SIDE, "mix_draw: sides up to %d", NVIT_AUG_MAX_SIDE);
  NVIT_REQUIRE(prob >= 0.f && prob <= 1.f && switch_prob >= 0.f && switch_prob <= 1.f, "mix_draw: probabilities in [0,1]");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * (MIX_ROW * 4.0 + 20.0), s);
  hipLaunchKernelGGL(mix_draw_kernel, dim3(1), dim3(256), 0, s, (unsigned long long)seed, (long long*)step,
                     (long long)first_index, q_mix, q_cut, prob, switch_prob, labels, table, lam, y2, B, H, W);
  NVIT_CHECK_LAUNCH("mix_draw");
  return NVIT_OK;
}

extern "C" int nvit_mix_apply(const float* in, const int* table, float* out, int B, int C, int H, int W, void* stream) {
  NVIT_REQUIRE(in && table && out && B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "mix_apply: bad arguments");
  NVIT_REQUIRE(W % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "mix_apply: needs W %% 4 == 0 and 16-byte aligned pointers");
  const long long n4 = (long long)C * H * (W / 4);
  NVIT_REQUIRE(n4 <= (1ll << 28), "mix_apply: image too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * (double)n4 * 32.0, s);
  const int chunks = (int)cdiv(n4, (long long)(MIX_THREADS * MIX_PER_THREAD));
  hipLaunchKernelGGL(mix_apply_kernel, dim3(chunks, B), dim3(MIX_THREADS), 0, s, in, table, out, B, (int)n4, H, W / 4);
  NVIT_CHECK_LAUNCH("mix_apply");
  return NVIT_OK;
}

extern "C" int nvit_augment_draw(const int* policy, int P, uint64_t seed, int64_t* step, int64_t first_index,
                                 const int* argtab, int* params, int B, void* stream) {
  NVIT_REQUIRE(policy && step && argtab && params && P > 0 && B > 0 && first_index >= 0,
               "augment_draw: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * 2.0 * AUG_ROW * 4.0, s);
  hipLaunchKernelGGL(augment_draw_kernel, dim3(1), dim3(256), 0, s, policy, P, (unsigned long long)seed,
                     (long long*)step, (long long)first_index, argtab, params, B);
  NVIT_CHECK_LAUNCH("augment_draw");
  return NVIT_OK;
}

extern "C" int nvit_randaug_draw(uint64_t seed, int64_t* step, int64_t first_index, const double* q, const double* rot,
                                 double magnitude, double mstd, double mmax, int increasing, float prob, int interp,
                                 double translate_pct, int* params, int B, int num_layers, int H, int W, void* stream) {
  NVIT_REQUIRE(step && q && rot && params && B > 0 && first_index >= 0 && ((uintptr_t)params & 7) == 0,
               "randaug_draw: bad arguments (the table is 8-byte aligned)");
  NVIT_REQUIRE(num_layers >= 1 && num_layers <= NVIT_RA_MAX_LAYERS && (long long)B * num_layers <= (1ll << 24),
               "randaug_draw: 1..%d layers", NVIT_RA_MAX_LAYERS);
  NVIT_REQUIRE(H > 0 && W > 0 && H <= NVIT_AUG_MAX_SIDE && W <= NVIT_AUG_MAX_SIDE, "randaug_draw: sides up to %d", NVIT_AUG_MAX_SIDE);
  // (the comparisons also refuse NaN; mstd may be +inf: timm's uniform magnitude)
  NVIT_REQUIRE(mmax > 0.0 && mmax <= 10.0 && magnitude >= 0.0 && magnitude <= 10.0 && mstd >= 0.0 && prob >= 0.f &&
                   prob <= 1.f && translate_pct >= 0.0 && translate_pct <= 1.0,
               "randaug_draw: needs 0 < mmax <= 10, 0 <= magnitude <= 10, mstd >= 0, prob and translate_pct in [0,1]");
  NVIT_REQUIRE(interp == NVIT_RA_BILINEAR || interp == NVIT_RA_BICUBIC || interp == NVIT_RA_RANDOM, "randaug_draw: unknown filter");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * num_layers * RA_ROW * 4.0, s);
  const double rot_scale = (double)RA_KNOTS / (3.0 * mmax);   // knots per degree: the table spans [0, 3 * mmax] degrees
  hipLaunchKernelGGL(randaug_draw_kernel, dim3(1), dim3(256), 0, s, (unsigned long long)seed, (long long*)step,
                     (long long)first_index, q, rot, magnitude, mstd, (int)(mstd > 1.7e308), mmax, increasing, prob, interp,
                     translate_pct, rot_scale, params, B, num_layers, H, W);
  NVIT_CHECK_LAUNCH("randaug_draw");
  return NVIT_OK;
}

extern "C" int nvit_randaug_apply(const void* in, const int* params, float* out_f32, void* out_u8, void* ws, int64_t ws_bytes,
                                  int B, int H, int W, int C, int num_layers, int fill0, int fill1, int fill2, float mean,
                                  float std_, void* stream) {
  NVIT_REQUIRE(in && params && ws && (out_f32 || out_u8) && B > 0 && H > 0 && W > 0 && (C == 1 || C == 3),
               "randaug_apply: bad arguments (C must be 1 or 3)");
  NVIT_REQUIRE(((uintptr_t)params & 7) == 0 && num_layers >= 1 && num_layers <= NVIT_RA_MAX_LAYERS,
               "randaug_apply: 1..%d layers and an 8-byte aligned table", NVIT_RA_MAX_LAYERS);
  NVIT_REQUIRE(H <= NVIT_AUG_MAX_SIDE && W <= NVIT_AUG_MAX_SIDE, "randaug_apply: sides up to %d", NVIT_AUG_MAX_SIDE);
  NVIT_REQUIRE(fill0 >= 0 && fill0 <= 255 && fill1 >= 0 && fill1 <= 255 && fill2 >= 0 && fill2 <= 255, "randaug_apply: fill 0..255");
  const size_t stride = ((size_t)H * W * C + 255) / 256 * 256;
  NVIT_REQUIRE(ws_bytes >= 0 && (size_t)ws_bytes >= 2 * (size_t)B * stride,
               "randaug_apply: workspace needs 2 * B * round_up(H*W*C, 256) bytes");
  if (out_f32) {
    NVIT_REQUIRE(W % 4 == 0 && std_ != 0.f && ((uintptr_t)out_f32 & 15) == 0,
                 "randaug_apply: fp32 output needs W %% 4 == 0, std != 0 and a 16-byte aligned pointer");
  }
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)B * H * W * C;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, n * (out_f32 ? 5.0 : 2.0), s);
  hipLaunchKernelGGL(randaug_apply_kernel, dim3(B), dim3(AUG_THREADS), 0, s, (const unsigned char*)in, params, out_f32,
                     (unsigned char*)out_u8, (unsigned char*)ws, stride, B, H, W, C, num_layers, fill0, fill1, fill2, mean,
                     1.0f / std_);
  NVIT_CHECK_LAUNCH("randaug_apply");
  return NVIT_OK;
}

extern "C" int nvit_augment_apply(const void* in, const int* params, float* out_f32, void* out_u8, void* ws,
                                  int64_t ws_bytes, int B, int H, int W, int C, float mean, float std_, void* stream) {
  NVIT_REQUIRE(in && params && ws && (out_f32 || out_u8) && B > 0 && H > 0 && W > 0 && (C == 1 || C == 3),
               "augment_apply: bad arguments (C must be 1 or 3)");
  // 16.16 coordinates and the 32-bit histogram sums stay in range
  NVIT_REQUIRE(H <= NVIT_AUG_MAX_SIDE && W <= NVIT_AUG_MAX_SIDE, "augment_apply: sides up to %d", NVIT_AUG_MAX_SIDE);
  const size_t stride = ((size_t)H * W * C + 255) / 256 * 256;
  NVIT_REQUIRE(ws_bytes >= 0 && (size_t)ws_bytes >= 2 * (size_t)B * stride,
               "augment_apply: workspace needs 2 * B * round_up(H*W*C, 256) bytes");
  if (out_f32) {
    NVIT_REQUIRE(W % 4 == 0 && std_ != 0.f && ((uintptr_t)out_f32 & 15) == 0,
                 "augment_apply: fp32 output needs W %% 4 == 0, std != 0 and a 16-byte aligned pointer");
  }
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)B * H * W * C;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, n * (out_f32 ? 5.0 : 2.0), s);
  hipLaunchKernelGGL(augment_apply_kernel, dim3(B), dim3(AUG_THREADS), 0, s, (const unsigned char*)in, params, out_f32,
                     (unsigned char*)out_u8, (unsigned char*)ws, stride, B, H, W, C, mean, 1.0f / std_);
  NVIT_CHECK_LAUNCH("augment_apply");
  return NVIT_OK;
}
