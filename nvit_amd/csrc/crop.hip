// On-device RandomResizedCrop + horizontal flip and RandomErasing: the per-image geometric half of the
// DeiT / timm recipe, in launches that a hipGraph can capture.  tests/crop_ref.py is the numpy twin.
//
//   nvit_crop_draw    one workgroup, one thread per image: torchvision's get_params in fp64 -> int32 [B,8] table
//   nvit_crop_apply   two launches, Pillow's two-pass 8-bit resampler on the box of each image:
//                       horizontal  grid (tile of output columns, image): the tile's taps, then box rows -> uint8 [h,size,C]
//                       vertical    grid (tile of output rows, image): the tile's taps, then the output, flip folded
//                                   into the store index
//   nvit_center_crop_apply   evaluation's Resize + CenterCrop, the same two passes on a window the host gives:
//                       horizontal  the window's columns of the source rows that its vertical taps read
//                       vertical    the window as uint8 [size,size,C] and / or normalised fp32 [C,size,size]
//   nvit_erase_draw   one workgroup, one thread per image: timm's RandomErasing box -> int32 [B,8] table
//   nvit_erase_apply  fp32 [B,C,H,W] -> fp32 [B,C,H,W], float4 streaming over (chunk of the image, image)
//
// The boxes differ per image, so the resampling coefficients are computed on the device, in fp64 and in Pillow's
// operation order; a tap set is computed once, by the workgroup that owns its output column (row), into the caller's
// workspace, and read back by that workgroup only.
#include "common.h"
#include "philox.h"

// Pillow's coefficients and the box draws are restated operation for operation: nothing in this file contracts.
#pragma clang fp contract(off)

namespace {

constexpr int CROP_ROW = NVIT_CROP_ROW;     // top, left, h, w, flip, 0, 0, 0
constexpr int ERASE_ROW = NVIT_ERASE_ROW;   // on, top, left, h, w, noise key low, noise key high, 0
constexpr int ATTEMPTS = NVIT_CROP_ATTEMPTS;
constexpr unsigned CROP_DOMAIN = 0x43524F50u;    // + attempt, xor-ed into the key's high word; + ATTEMPTS: the flip
constexpr unsigned ERASE_DOMAIN = 0x45524153u;   // + attempt; + ATTEMPTS: the gate; + ATTEMPTS + 1: the noise sub-key
constexpr int PRECISION_BITS = 22;               // Pillow: 32 - 8 - 2
constexpr int CROP_THREADS = 256;
constexpr int CROP_TILE = 16;   // output columns (horizontal pass) or rows (vertical pass) per workgroup
__device__ __forceinline__ Philox4 draw_words(unsigned long long g, unsigned long long step, unsigned long long seed,
                                              unsigned domain) {
  return philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                       (unsigned)(seed >> 32) ^ domain);
}
__device__ __forceinline__ double unit64(unsigned r) { return (double)(r >> 8) * 0x1p-24; }
// exp(U(log lo, log hi)) from the host's table: top 10 bits pick the knot, the next 14 interpolate
__device__ __forceinline__ double aspect_of(const double* __restrict__ t, unsigned r) {
  const unsigned u = r >> 8;
  const int k = (int)(u >> 14);
  const double f = (double)(u & 0x3FFFu) * 0x1p-14;
  return t[k] + f * (t[k + 1] - t[k]);
}
__device__ __forceinline__ int int_range(unsigned r, int n) { return (int)(((unsigned long long)r * (unsigned long long)n) >> 32); }

__global__ __launch_bounds__(256) void crop_draw_kernel(unsigned long long seed, long long* step_ctr, long long first_index,
                                                        const double* __restrict__ aspect, double s0, double s1,
                                                        double rmin, double rmax, float hflip, int* __restrict__ table,
                                                        int B, int Hs, int Ws) {
  const unsigned long long step = (unsigned long long)*step_ctr;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const unsigned long long g = (unsigned long long)(first_index + i);
    int top = 0, left = 0, h = 0, w = 0;
    bool done = false;
    for (int a = 0; a < ATTEMPTS && !done; ++a) {
      const Philox4 r = draw_words(g, step, seed, CROP_DOMAIN + (unsigned)a);
      const double target = (double)(Hs * Ws) * (s0 + unit64(r.v[0]) * (s1 - s0));
      const double asp = aspect_of(aspect, r.v[1]);
      const double wd = rint(__dsqrt_rn(target * asp)), hd = rint(__dsqrt_rn(target / asp));
      if (wd > 0.0 && wd <= (double)Ws && hd > 0.0 && hd <= (double)Hs) {
        w = (int)wd;
        h = (int)hd;
        top = int_range(r.v[2], Hs - h + 1);
        left = int_range(r.v[3], Ws - w + 1);
        done = true;
      }
    }
    if (!done) {   // torchvision's central crop
      const double in_ratio = (double)Ws / (double)Hs;
      double hd = (double)Hs, wd = (double)Ws;
      if (in_ratio < rmin) {
        hd = rint((double)Ws / rmin);
      } else if (in_ratio > rmax) {
        wd = rint((double)Hs * rmax);
      }
      hd = hd < 1.0 ? 1.0 : (hd > (double)Hs ? (double)Hs : hd);   // (a ratio so extreme that a side rounds to 0)
      wd = wd < 1.0 ? 1.0 : (wd > (double)Ws ? (double)Ws : wd);
      h = (int)hd;
      w = (int)wd;
      top = (Hs - h) / 2;
      left = (Ws - w) / 2;
    }
    const Philox4 rf = draw_words(g, step, seed, CROP_DOMAIN + (unsigned)ATTEMPTS);
    int* row = table + (size_t)i * CROP_ROW;
    row[0] = top;
    row[1] = left;
    row[2] = h;
    row[3] = w;
    row[4] = (float)(rf.v[0] >> 8) * 0x1p-24f < hflip ? 1 : 0;
    row[5] = 0;
    row[6] = 0;
    row[7] = 0;
  }
  __syncthreads();   // every thread has read the counter
  if (threadIdx.x == 0) *step_ctr = (long long)(step + 1);
}

// ------------------------------------------------------------------------------------------------ Pillow's resampler
struct CropBox {
  int top, left, h, w;
  bool flip;
};
// the box of a table row; one that leaves the image is the whole image, so no table sends a kernel out of bounds
__device__ __forceinline__ CropBox box_of(const int* __restrict__ row, int Hs, int Ws) {
  CropBox b{row[0], row[1], row[2], row[3], row[4] != 0};
  const bool ok = b.h >= 1 && b.w >= 1 && b.top >= 0 && b.left >= 0 && b.h <= Hs && b.w <= Ws && b.top <= Hs - b.h &&
                  b.left <= Ws - b.w;
  if (!ok) {
    b.top = 0;
    b.left = 0;
    b.h = Hs;
    b.w = Ws;
  }
  return b;
}

__device__ __forceinline__ double resample_filter(double x, int interp) {
  x = x < 0.0 ? -x : x;
  if (interp == NVIT_CROP_BICUBIC) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;
}

// ints per tap set: first input index, number of taps, then kstride taps
__host__ __device__ inline int set_stride(int kstride) { return kstride + 2; }

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output index xx of an axis in_size -> out_size.  The weights
// are evaluated twice (sum, then normalise) instead of stored: the same expression gives the same double.
__device__ void tap_set(int* set, int kstride, int xx, int in_size, int out_size, int interp) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (interp == NVIT_CROP_BICUBIC ? 2.0 : 1.0) * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  xmin = xmin < 0 ? 0 : xmin;
  int xmax = (int)(center + support + 0.5);
  xmax = xmax > in_size ? in_size : xmax;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > kstride ? kstride : n);   // n <= 2 * ceil(support) + 1 <= kstride: the clamp never acts
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += resample_filter(((double)(x + xmin) - center + 0.5) * ss, interp);
  set[0] = xmin;
  set[1] = n;
  for (int x = 0; x < n; ++x) {
    double w = resample_filter(((double)(x + xmin) - center + 0.5) * ss, interp);
    if (ww != 0.0) w = w / ww;
    set[2 + x] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
  }
}

__device__ __forceinline__ unsigned clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The body of both horizontal passes: `rows` source rows of Ws pixels -> columns c0 .. c0 + ncols - 1 of `rows` rows of
// `size` pixels, by this workgroup's tap sets.  One thread per (row, output column): a tap is loaded once for the pixel's
// channels.
__device__ __forceinline__ void resample_rows(const unsigned char* src, unsigned char* dst, const int* sets, int st,
                                              int rows, int ncols, int c0, int Ws, int C, int size) {
  const int total = rows * ncols;
  for (int i = threadIdx.x; i < total; i += CROP_THREADS) {
    const int y = i / ncols, xc = i - y * ncols;
    const int* set = sets + (size_t)xc * st;
    const int xmin = set[0], n = set[1];
    const unsigned char* p = src + ((size_t)y * Ws + xmin) * C;   // xmin + n <= w: inside the box
    unsigned char* o = dst + ((size_t)y * size + c0 + xc) * C;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    if (C == 3) {
      for (int x = 0; x < n; ++x) {
        const int t = set[2 + x];
        a0 += t * (int)p[3 * x];
        a1 += t * (int)p[3 * x + 1];
        a2 += t * (int)p[3 * x + 2];
      }
      o[0] = (unsigned char)clip8(a0);
      o[1] = (unsigned char)clip8(a1);
      o[2] = (unsigned char)clip8(a2);
    } else {
      for (int x = 0; x < n; ++x) a0 += set[2 + x] * (int)p[x];
      o[0] = (unsigned char)clip8(a0);
    }
  }
}

// taps: int32 [B,2,size,set_stride(kstride)] (axis 0 horizontal, 1 vertical); mid: uint8 [B,Hs,size,C], rows 0..h-1 used.
__global__ __launch_bounds__(CROP_THREADS) void crop_h_kernel(const unsigned char* __restrict__ in,
                                                              const int* __restrict__ table, int* taps,
                                                              unsigned char* __restrict__ mid, int Hs, int Ws, int C,
                                                              int size, int kstride, int interp) {
  const int b = blockIdx.y, c0 = blockIdx.x * CROP_TILE;
  const int ncols = size - c0 < CROP_TILE ? size - c0 : CROP_TILE;
  const CropBox bx = box_of(table + (size_t)b * CROP_ROW, Hs, Ws);
  const int st = set_stride(kstride);
  int* sets = taps + (((size_t)b * 2 + 0) * size + c0) * st;
  if ((int)threadIdx.x < ncols) tap_set(sets + (size_t)threadIdx.x * st, kstride, c0 + threadIdx.x, bx.w, size, interp);
  __syncthreads();   // this workgroup's tap sets are in memory (a workgroup-scope release/acquire)
  const unsigned char* src = in + (((size_t)b * Hs + bx.top) * Ws + bx.left) * C;
  unsigned char* dst = mid + (size_t)b * Hs * size * C;
  resample_rows(src, dst, sets, st, bx.h, ncols, c0, Ws, C, size);
}

__global__ __launch_bounds__(CROP_THREADS) void crop_v_kernel(const unsigned char* __restrict__ mid,
                                                              const int* __restrict__ table, int* taps,
                                                              unsigned char* __restrict__ out, int Hs, int Ws, int C,
                                                              int size, int kstride, int interp) {
  const int b = blockIdx.y, r0 = blockIdx.x * CROP_TILE;
  const int nrows = size - r0 < CROP_TILE ? size - r0 : CROP_TILE;
  const CropBox bx = box_of(table + (size_t)b * CROP_ROW, Hs, Ws);
  const int st = set_stride(kstride);
  int* sets = taps + (((size_t)b * 2 + 1) * size + r0) * st;
  if ((int)threadIdx.x < nrows) tap_set(sets + (size_t)threadIdx.x * st, kstride, r0 + threadIdx.x, bx.h, size, interp);
  __syncthreads();
  const int row_b = size * C, q4 = row_b / 4;   // size % 4 == 0: a row is whole 4-byte words
  const unsigned char* src = mid + (size_t)b * Hs * row_b;
  for (int i = threadIdx.x; i < nrows * q4; i += CROP_THREADS) {
    const int ry = i / q4, j = i - ry * q4;
    const int* set = sets + (size_t)ry * st;
    const int ymin = set[0], n = set[1];
    int acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < n; ++y) {   // ymin + n <= h: rows the horizontal pass wrote
      const unsigned v = *reinterpret_cast<const unsigned*>(src + (size_t)(ymin + y) * row_b + 4 * j);
      const int t = set[2 + y];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += t * (int)((v >> (8 * e)) & 255u);
    }
    unsigned char* orow = out + ((size_t)b * size + r0 + ry) * row_b;
    if (!bx.flip) {
      // The four bytes are assembled with v_perm_b32.  Written as shifts and ors, hipcc fuses shift, clamp and pack of
      // two of them into v_ashr_pk_u8_i32 and ors the other two into its result as if the upper half were zero; on the
      // MI355X it was not.
      const unsigned lo = __builtin_amdgcn_perm(clip8(acc[1]), clip8(acc[0]), 0x0c0c0400u);
      const unsigned hi = __builtin_amdgcn_perm(clip8(acc[3]), clip8(acc[2]), 0x04000c0cu);
      *reinterpret_cast<unsigned*>(orow + 4 * j) = lo | hi;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = 4 * j + e, col = idx / C, ch = idx - col * C;
        orow[(size - 1 - col) * C + ch] = (unsigned char)clip8(acc[e]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ Resize + CenterCrop
// Evaluation's transform: every image is resampled to a virtual [H2,W2] and only the size x size window at (top, left)
// of it is computed.  The geometry is the host's, one per batch.  A window is the whole resize with the output index
// shifted, tap_set(left + j, Ws, W2): resizing and then cutting gives the same bytes (tests/center_crop_ref.py).
struct CenterGeom {
  int Hs, Ws, H2, W2, top, left, size, interp;
  int row0, nrows;    // the source rows that the window's vertical taps read: row0 .. row0 + nrows - 1
  int kst_w, kst_h;   // taps per set of each axis
};

// taps: int32 [B,size,set_stride(kst_w)]; mid: uint8 [B,nrows,size,C], source rows row0 .. of the window's columns.
__global__ __launch_bounds__(CROP_THREADS) void center_h_kernel(const unsigned char* __restrict__ in, int* taps,
                                                                unsigned char* __restrict__ mid, int C, CenterGeom g) {
  const int b = blockIdx.y, c0 = blockIdx.x * CROP_TILE;
  const int ncols = g.size - c0 < CROP_TILE ? g.size - c0 : CROP_TILE;
  const int st = set_stride(g.kst_w);
  int* sets = taps + ((size_t)b * g.size + c0) * st;
  if ((int)threadIdx.x < ncols)
    tap_set(sets + (size_t)threadIdx.x * st, g.kst_w, g.left + c0 + threadIdx.x, g.Ws, g.W2, g.interp);
  __syncthreads();   // this workgroup's tap sets are in memory (a workgroup-scope release/acquire)
  const unsigned char* src = in + ((size_t)b * g.Hs + g.row0) * g.Ws * C;   // xmin + n <= Ws: inside the image
  unsigned char* dst = mid + (size_t)b * g.nrows * g.size * C;
  resample_rows(src, dst, sets, st, g.nrows, ncols, c0, g.Ws, C, g.size);
}

// ToTensor + Normalize of one byte with nvit_normalize_images' roundings.  rowops.hip compiles (x * (1/255) - mean) *
// inv_std under the default contraction, which fuses the first two; this file contracts nothing, so the fusion is written.
__device__ __forceinline__ float normalize1(unsigned x, float mean, float inv_std) {
  return __builtin_fmaf((float)x, 1.0f / 255.0f, -mean) * inv_std;
}

// taps: int32 [B,size,set_stride(kst_h)].  A thread owns four neighbouring pixels of an output row, C 4-byte words of
// the HWC intermediate: packed, they are C words of the uint8 output; taken apart by channel, one float4 of each of the C
// planes of the fp32 output, so that neighbouring threads store neighbouring 16 bytes of a plane's row.
template <int C>
__global__ __launch_bounds__(CROP_THREADS) void center_v_kernel(const unsigned char* __restrict__ mid, int* taps,
                                                                unsigned char* __restrict__ out_u8,
                                                                float* __restrict__ out_f32, CenterGeom g, float mean,
                                                                float inv_std) {
  const int b = blockIdx.y, r0 = blockIdx.x * CROP_TILE;
  const int nrows = g.size - r0 < CROP_TILE ? g.size - r0 : CROP_TILE;
  const int st = set_stride(g.kst_h);
  int* sets = taps + ((size_t)b * g.size + r0) * st;
  if ((int)threadIdx.x < nrows)
    tap_set(sets + (size_t)threadIdx.x * st, g.kst_h, g.top + r0 + threadIdx.x, g.Hs, g.H2, g.interp);
  __syncthreads();
  const int row_b = g.size * C, q = g.size / 4;   // size % 4 == 0
  const unsigned char* src = mid + (size_t)b * g.nrows * row_b;
  for (int i = threadIdx.x; i < nrows * q; i += CROP_THREADS) {
    const int ry = i / q, j = i - ry * q;
    const int* set = sets + (size_t)ry * st;
    const int y0 = set[0] - g.row0;
    // the host found row0 and nrows with tap_set's own expressions, so the test never fails; it keeps every read inside
    const int n = y0 >= 0 && y0 + set[1] <= g.nrows ? set[1] : 0;
    int acc[4 * C];
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) acc[k] = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < n; ++y) {
      const unsigned* p = reinterpret_cast<const unsigned*>(src + (size_t)(y0 + y) * row_b) + C * j;
      const int t = set[2 + y];
#pragma unroll
      for (int w = 0; w < C; ++w) {
        const unsigned v = p[w];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * w + e] += t * (int)((v >> (8 * e)) & 255u);
      }
    }
    unsigned px[4 * C];   // byte k = channel k % C of pixel k / C
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) px[k] = clip8(acc[k]);
    if (out_u8) {
      unsigned* o = reinterpret_cast<unsigned*>(out_u8 + ((size_t)b * g.size + r0 + ry) * row_b) + C * j;
#pragma unroll
      for (int w = 0; w < C; ++w)   // v_perm_b32, as in crop_v_kernel
        o[w] = __builtin_amdgcn_perm(px[4 * w + 1], px[4 * w], 0x0c0c0400u) |
               __builtin_amdgcn_perm(px[4 * w + 3], px[4 * w + 2], 0x04000c0cu);
    }
    if (out_f32) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = normalize1(px[e * C + c], mean, inv_std);
        *reinterpret_cast<f32x4*>(out_f32 + (((size_t)b * C + c) * g.size + r0 + ry) * g.size + 4 * j) = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ RandomErasing
__global__ __launch_bounds__(256) void erase_draw_kernel(unsigned long long seed, long long* step_ctr, long long first_index,
                                                         const double* __restrict__ aspect, double a0, double a1, float prob,
                                                         int* __restrict__ table, int B, int H, int W) {
  const unsigned long long step = (unsigned long long)*step_ctr;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const unsigned long long g = (unsigned long long)(first_index + i);
    const Philox4 rg = draw_words(g, step, seed, ERASE_DOMAIN + (unsigned)ATTEMPTS);
    const bool gate = (float)(rg.v[0] >> 8) * 0x1p-24f < prob;
    int on = 0, top = 0, left = 0, h = 0, w = 0;
    for (int a = 0; a < ATTEMPTS && gate && !on; ++a) {
      const Philox4 r = draw_words(g, step, seed, ERASE_DOMAIN + (unsigned)a);
      const double target = (double)(H * W) * (a0 + unit64(r.v[0]) * (a1 - a0));
      const double asp = aspect_of(aspect, r.v[1]);
      const double hd = rint(__dsqrt_rn(target * asp)), wd = rint(__dsqrt_rn(target / asp));
      if (wd < (double)W && hd < (double)H) {   // timm's strict <
        h = (int)hd;
        w = (int)wd;
        top = int_range(r.v[2], H - h + 1);
        left = int_range(r.v[3], W - w + 1);
        on = 1;
      }
    }
    const Philox4 rk = draw_words(g, step, seed, ERASE_DOMAIN + (unsigned)ATTEMPTS + 1u);
    int* row = table + (size_t)i * ERASE_ROW;
    row[0] = on;
    row[1] = top;
    row[2] = left;
    row[3] = h;
    row[4] = w;
    row[5] = (int)rk.v[0];
    row[6] = (int)rk.v[1];
    row[7] = 0;
  }
  __syncthreads();   // every thread has read the counter
  if (threadIdx.x == 0) *step_ctr = (long long)(step + 1);
}

constexpr int ERASE_THREADS = 256;
constexpr int ERASE_PER_THREAD = 4;

// Grid (chunks of an image, images).  Every float4 is read and written by one thread, so out == in is allowed; in place
// only the float4s that touch the box are read at all.
__global__ __launch_bounds__(ERASE_THREADS) void erase_apply_kernel(const float* in, const int* __restrict__ table,
                                                                    const float* __restrict__ q, float* out, int mode,
                                                                    int n4, int H, int w4) {
  const int b = blockIdx.y;
  const int* row = table + (size_t)b * ERASE_ROW;
  const int top = row[1], left = row[2], h = row[3], w = row[4], W = w4 * 4;
  const bool erase = row[0] != 0 && h >= 1 && w >= 1 && top >= 0 && left >= 0 && h <= H && w <= W && top <= H - h &&
                     left <= W - w;
  const unsigned k0 = (unsigned)row[5], k1 = (unsigned)row[6];
  const f32x4* src = reinterpret_cast<const f32x4*>(in + (size_t)b * n4 * 4);
  f32x4* dst = reinterpret_cast<f32x4*>(out + (size_t)b * n4 * 4);
  const int base = blockIdx.x * (ERASE_THREADS * ERASE_PER_THREAD) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < ERASE_PER_THREAD; ++k) {
    const int i = base + k * ERASE_THREADS;
    if (i >= n4) continue;
    const int x = (i % w4) * 4, y = (i / w4) % H;
    const bool touch = erase && y >= top && y < top + h && x + 3 >= left && x < left + w;
    if (!touch) {
      if (in != out) dst[i] = src[i];
      continue;
    }
    const f32x4 v = src[i];
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (mode == NVIT_ERASE_PIXEL) {
      const Philox4 r = philox4x32_10((unsigned)i, 0u, 0u, 0u, k0, k1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned u = r.v[e] >> 8;
        const int kn = (int)(u >> 14);
        const float f = (float)(u & 0x3FFFu) * 0x1p-14f;   // exact
        z[e] = q[kn] + f * (q[kn + 1] - q[kn]);            // three roundings (file-wide contract(off))
      }
    }
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (x + e >= left && x + e < left + w) ? z[e] : v[e];
    dst[i] = o;
  }
}

// taps per set for the largest box of an axis: Pillow's ksize = 2 * ceil(support) + 1
int crop_kstride(int Hs, int Ws, int size, int interp) {
  const int side = Hs > Ws ? Hs : Ws;
  const double scale = (double)side / (double)size;
  const double support = (interp == NVIT_CROP_BICUBIC ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}
size_t crop_taps_bytes(int B, int Hs, int Ws, int size, int interp) {
  const size_t n = (size_t)B * 2 * size * set_stride(crop_kstride(Hs, Ws, size, interp)) * sizeof(int);
  return (n + 255) / 256 * 256;
}
bool crop_shape_ok(int B, int Hs, int Ws, int C, int size, int interp) {
  return B > 0 && B <= NVIT_CROP_MAX_BATCH && Hs > 0 && Ws > 0 && Hs <= NVIT_CROP_MAX_SRC && Ws <= NVIT_CROP_MAX_SRC && (C == 1 || C == 3) &&
         size > 0 && size <= NVIT_AUG_MAX_SIDE && size % 4 == 0 && (interp == NVIT_CROP_BILINEAR || interp == NVIT_CROP_BICUBIC);
}


// ---- Resize + CenterCrop: the host's half
int axis_kstride(int in_size, int out_size, int interp) {
  const double scale = (double)in_size / (double)out_size;
  const double support = (interp == NVIT_CROP_BICUBIC ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}
// [first, end) of the input indices that the taps of output index xx read: tap_set's expressions, in fp64 like them
// (the pragma above covers the host's code too).  Both ends grow with xx.
void tap_range(int xx, int in_size, int out_size, int interp, int* first, int* end) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (interp == NVIT_CROP_BICUBIC ? 2.0 : 1.0) * fs;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  xmin = xmin < 0 ? 0 : xmin;
  int xmax = (int)(center + support + 0.5);
  xmax = xmax > in_size ? in_size : xmax;
  *first = xmin;
  *end = xmax < xmin ? xmin : xmax;
}
bool center_shape_ok(int B, int Hs, int Ws, int C, int H2, int W2, int top, int left, int size, int interp) {
  return B > 0 && B <= NVIT_CROP_MAX_BATCH && Hs > 0 && Ws > 0 && Hs <= NVIT_CROP_MAX_SRC && Ws <= NVIT_CROP_MAX_SRC &&
         (C == 1 || C == 3) && size >= 4 && size <= NVIT_AUG_MAX_SIDE && size % 4 == 0 && H2 <= NVIT_AUG_MAX_SIDE &&
         W2 <= NVIT_AUG_MAX_SIDE && H2 >= size && W2 >= size && top >= 0 && top <= H2 - size && left >= 0 &&
         left <= W2 - size && (interp == NVIT_CROP_BILINEAR || interp == NVIT_CROP_BICUBIC);
}
CenterGeom center_geom(int Hs, int Ws, int H2, int W2, int top, int left, int size, int interp) {
  CenterGeom g{Hs, Ws, H2, W2, top, left, size, interp, 0, 0, axis_kstride(Ws, W2, interp), axis_kstride(Hs, H2, interp)};
  int first, end, unused;
  tap_range(top, Hs, H2, interp, &first, &unused);
  tap_range(top + size - 1, Hs, H2, interp, &unused, &end);
  g.row0 = first;
  g.nrows = end - first;
  return g;
}
// the two tap tables, each rounded up to 256 bytes: the horizontal one, then the vertical one, then the intermediate
size_t center_taps_bytes(int B, const CenterGeom& g, int kst) {
  return ((size_t)B * g.size * set_stride(kst) * sizeof(int) + 255) / 256 * 256;
}

}  // namespace

extern "C" int64_t nvit_center_crop_ws_bytes(int B, int Hs, int Ws, int C, int H2, int W2, int top, int left, int size,
                                             int interp) {
  if (!center_shape_ok(B, Hs, Ws, C, H2, W2, top, left, size, interp)) return -1;
  const CenterGeom g = center_geom(Hs, Ws, H2, W2, top, left, size, interp);
  return (int64_t)(center_taps_bytes(B, g, g.kst_w) + center_taps_bytes(B, g, g.kst_h) + (size_t)B * g.nrows * size * C);
}

extern "C" int nvit_center_crop_apply(const void* in, void* out_u8, float* out_f32, void* ws, int64_t ws_bytes, int B, int Hs,
                                      int Ws, int C, int H2, int W2, int top, int left, int size, int interp, float mean,
                                      float std_, void* stream) {
  NVIT_REQUIRE(in && ws && (out_u8 || out_f32), "center_crop_apply: bad arguments (at least one output)");
  NVIT_REQUIRE(center_shape_ok(B, Hs, Ws, C, H2, W2, top, left, size, interp),
               "center_crop_apply: needs C in {1,3}, source sides up to %d, size %% 4 == 0 in 4..%d, size <= H2, W2 <= %d, "
               "0 <= top <= H2 - size, 0 <= left <= W2 - size, B up to %d and a known filter",
               NVIT_CROP_MAX_SRC, NVIT_AUG_MAX_SIDE, NVIT_AUG_MAX_SIDE, NVIT_CROP_MAX_BATCH);
  NVIT_REQUIRE(!out_f32 || std_ > 0.f, "center_crop_apply: std must be positive");
  NVIT_REQUIRE(ws_bytes >= nvit_center_crop_ws_bytes(B, Hs, Ws, C, H2, W2, top, left, size, interp),
               "center_crop_apply: workspace needs nvit_center_crop_ws_bytes(...) bytes");
  NVIT_REQUIRE(((uintptr_t)out_u8 & 3) == 0 && ((uintptr_t)out_f32 & 15) == 0 && ((uintptr_t)ws & 15) == 0,
               "center_crop_apply: out_u8 4-byte, out_f32 and ws 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const CenterGeom g = center_geom(Hs, Ws, H2, W2, top, left, size, interp);
  int* taps_w = (int*)ws;
  int* taps_h = (int*)((unsigned char*)ws + center_taps_bytes(B, g, g.kst_w));
  unsigned char* mid = (unsigned char*)taps_h + center_taps_bytes(B, g, g.kst_h);
  const double px = (double)B * C, out_b = (out_u8 ? 1.0 : 0.0) + (out_f32 ? 4.0 : 0.0);
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, px * ((double)g.nrows * Ws + 2.0 * g.nrows * size + out_b * size * size), s);
  const dim3 grid(cdiv(size, CROP_TILE), B);
  hipLaunchKernelGGL(center_h_kernel, grid, dim3(CROP_THREADS), 0, s, (const unsigned char*)in, taps_w, mid, C, g);
  NVIT_CHECK_LAUNCH("center_crop_apply (horizontal)");
  const float inv_std = out_f32 ? 1.0f / std_ : 0.f;
  if (C == 3)
    hipLaunchKernelGGL(center_v_kernel<3>, grid, dim3(CROP_THREADS), 0, s, (const unsigned char*)mid, taps_h,
                       (unsigned char*)out_u8, out_f32, g, mean, inv_std);
  else
    hipLaunchKernelGGL(center_v_kernel<1>, grid, dim3(CROP_THREADS), 0, s, (const unsigned char*)mid, taps_h,
                       (unsigned char*)out_u8, out_f32, g, mean, inv_std);
  NVIT_CHECK_LAUNCH("center_crop_apply (vertical)");
  return NVIT_OK;
}

extern "C" int nvit_crop_draw(uint64_t seed, int64_t* step, int64_t first_index, const double* aspect, double scale0,
                              double scale1, double ratio_min, double ratio_max, float hflip, int* table, int B, int Hs,
                              int Ws, void* stream) {
  NVIT_REQUIRE(step && aspect && table && B > 0 && first_index >= 0, "crop_draw: bad arguments");
  NVIT_REQUIRE(Hs > 0 && Ws > 0 && Hs <= NVIT_CROP_MAX_SRC && Ws <= NVIT_CROP_MAX_SRC, "crop_draw: source sides up to %d",
               NVIT_CROP_MAX_SRC);
  NVIT_REQUIRE(scale0 > 0.0 && scale0 <= scale1 && ratio_min > 0.0 && ratio_min <= ratio_max && hflip >= 0.f && hflip <= 1.f,
               "crop_draw: 0 < scale0 <= scale1, 0 < ratio_min <= ratio_max and hflip in [0,1]");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * CROP_ROW * 4.0, s);
  hipLaunchKernelGGL(crop_draw_kernel, dim3(1), dim3(256), 0, s, (unsigned long long)seed, (long long*)step,
                     (long long)first_index, aspect, scale0, scale1, ratio_min, ratio_max, hflip, table, B, Hs, Ws);
  NVIT_CHECK_LAUNCH("crop_draw");
  return NVIT_OK;
}

extern "C" int64_t nvit_crop_ws_bytes(int B, int Hs, int Ws, int C, int size, int interp) {
  if (!crop_shape_ok(B, Hs, Ws, C, size, interp)) return -1;
  return (int64_t)(crop_taps_bytes(B, Hs, Ws, size, interp) + (size_t)B * Hs * size * C);
}

extern "C" int nvit_crop_apply(const void* in, const int* table, void* out, void* ws, int64_t ws_bytes, int B, int Hs, int Ws,
                               int C, int size, int interp, void* stream) {
  NVIT_REQUIRE(in && table && out && ws, "crop_apply: bad arguments");
  NVIT_REQUIRE(crop_shape_ok(B, Hs, Ws, C, size, interp),
               "crop_apply: needs C in {1,3}, source sides up to %d, size %% 4 == 0 up to %d, B up to %d and a known filter",
               NVIT_CROP_MAX_SRC, NVIT_AUG_MAX_SIDE, NVIT_CROP_MAX_BATCH);
  NVIT_REQUIRE(ws_bytes >= nvit_crop_ws_bytes(B, Hs, Ws, C, size, interp), "crop_apply: workspace needs nvit_crop_ws_bytes(...) bytes");
  NVIT_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)ws & 15) == 0, "crop_apply: out 4-byte and ws 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int kstride = crop_kstride(Hs, Ws, size, interp);
  int* taps = (int*)ws;
  unsigned char* mid = (unsigned char*)ws + crop_taps_bytes(B, Hs, Ws, size, interp);
  const double px = (double)B * C;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, px * ((double)Hs * Ws + 2.0 * Hs * size + (double)size * size), s);
  const dim3 grid(cdiv(size, CROP_TILE), B);
  hipLaunchKernelGGL(crop_h_kernel, grid, dim3(CROP_THREADS), 0, s, (const unsigned char*)in, table, taps, mid, Hs, Ws, C, size,
                     kstride, interp);
  NVIT_CHECK_LAUNCH("crop_apply (horizontal)");
  hipLaunchKernelGGL(crop_v_kernel, grid, dim3(CROP_THREADS), 0, s, (const unsigned char*)mid, table, taps,
                     (unsigned char*)out, Hs, Ws, C, size, kstride, interp);
  NVIT_CHECK_LAUNCH("crop_apply (vertical)");
  return NVIT_OK;
}

extern "C" int nvit_erase_draw(uint64_t seed, int64_t* step, int64_t first_index, const double* aspect, double area0,
                               double area1, float prob, int* table, int B, int H, int W, void* stream) {
  NVIT_REQUIRE(step && aspect && table && B > 0 && first_index >= 0, "erase_draw: bad arguments");
  NVIT_REQUIRE(H > 0 && W > 0 && H <= NVIT_AUG_MAX_SIDE && W <= NVIT_AUG_MAX_SIDE, "erase_draw: sides up to %d", NVIT_AUG_MAX_SIDE);
  NVIT_REQUIRE(area0 > 0.0 && area0 <= area1 && prob >= 0.f && prob <= 1.f, "erase_draw: 0 < area0 <= area1 and prob in [0,1]");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * ERASE_ROW * 4.0, s);
  hipLaunchKernelGGL(erase_draw_kernel, dim3(1), dim3(256), 0, s, (unsigned long long)seed, (long long*)step,
                     (long long)first_index, aspect, area0, area1, prob, table, B, H, W);
  NVIT_CHECK_LAUNCH("erase_draw");
  return NVIT_OK;
}

extern "C" int nvit_erase_apply(const float* in, const int* table, const float* q, float* out, int mode, int B, int C, int H,
                                int W, void* stream) {
  NVIT_REQUIRE(in && table && out && B > 0 && B <= NVIT_CROP_MAX_BATCH && C > 0 && H > 0 && W > 0, "erase_apply: bad arguments");
  NVIT_REQUIRE(mode == NVIT_ERASE_CONST || (mode == NVIT_ERASE_PIXEL && q), "erase_apply: mode 0 (const) or 1 (pixel, with its table)");
  NVIT_REQUIRE(W % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "erase_apply: needs W %% 4 == 0 and 16-byte aligned pointers");
  NVIT_REQUIRE(H <= NVIT_AUG_MAX_SIDE && W <= NVIT_AUG_MAX_SIDE, "erase_apply: sides up to %d", NVIT_AUG_MAX_SIDE);
  const long long n4 = (long long)C * H * (W / 4);
  NVIT_REQUIRE(n4 <= (1ll << 28), "erase_apply: image too large");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * (double)n4 * (in == out ? 8.0 : 32.0), s);
  const int chunks = (int)cdiv(n4, (long long)(ERASE_THREADS * ERASE_PER_THREAD));
  hipLaunchKernelGGL(erase_apply_kernel, dim3(chunks, B), dim3(ERASE_THREADS), 0, s, in, table, q, out, mode, (int)n4, H, W / 4);
  NVIT_CHECK_LAUNCH("erase_apply");
  return NVIT_OK;
}
