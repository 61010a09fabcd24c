// Position-embedding resampling (timm's resample_abs_pos_embed; nvit_amd/resample.py is the host side):
//   nvit_pos_resample_fwd   p [g*g, C] -> out [g2*g2, C], bicubic (a = -0.5), antialiased, align_corners = false
//   nvit_pos_resample_bwd   its exact adjoint, d [g2*g2, C] -> grad [g*g, C]
// The operator is separable, out = (W (x) W) p, and W's rows are short (4 taps enlarging, 4 * g / g2 shrinking).  Both
// directions are ONE gather kernel: a destination row (dy, dx) reads the source rows (y0 + ty, x0 + tx) named by two rows of a
// tap table the host computed in fp64 - W for the forward, W^T for the backward - so every destination element is written
// once, by one lane, in a fixed order: no atomics, no memset.  One wave per destination row, float4 over C, the grid of the
// forward row kernels (rowops.hip).  The tables are a few KB of launch-latency-bound work: no LDS, no tiling.
#include "common.h"

namespace {

constexpr int ROW_WAVES = NVIT_ROW_WAVES;
constexpr int MAX_TAPS = NVIT_POS_RESAMPLE_MAX_TAPS;
constexpr int TAP_ROW = 2 + MAX_TAPS;   // (first, count, weights...)

// (first, count) of a table row, clipped to the source grid: a damaged table reads wrong values, never outside src.
__device__ __forceinline__ void tap_span(const int* __restrict__ row, int n_src, int& first, int& count) {
  first = min(max(row[0], 0), n_src - 1);
  count = min(max(row[1], 0), min(MAX_TAPS, n_src - first));
}

template <bool TWO>
__global__ __launch_bounds__(256) void pos_resample_kernel(const float* __restrict__ src0, const float* __restrict__ src1,
                                                           const int* __restrict__ taps, float* __restrict__ dst0,
                                                           float* __restrict__ dst1, int n_src, int n_dst, int C4) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int rows = n_dst * n_dst;
  for (int r = blockIdx.x * ROW_WAVES + wid; r < rows; r += gridDim.x * ROW_WAVES) {
    const int dy = r / n_dst, dx = r - dy * n_dst;
    const int* __restrict__ ty = taps + (size_t)dy * TAP_ROW;
    const int* __restrict__ tx = taps + (size_t)dx * TAP_ROW;
    int y0, ny, x0, nx;
    tap_span(ty, n_src, y0, ny);
    tap_span(tx, n_src, x0, nx);
    const size_t dofs = (size_t)r * C4 * 4;
    for (int c = lane; c < C4; c += 64) {
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
      for (int iy = 0; iy < ny; ++iy) {
        const float wy = __int_as_float(ty[2 + iy]);
        const size_t so = ((size_t)(y0 + iy) * n_src + x0) * C4 * 4 + 4 * c;
        for (int ix = 0; ix < nx; ++ix) {
          const float w = wy * __int_as_float(tx[2 + ix]);
          const f32x4 v0 = load4<float>(src0 + so + (size_t)ix * C4 * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) a0[e] = __builtin_fmaf(w, v0[e], a0[e]);
          if constexpr (TWO) {
            const f32x4 v1 = load4<float>(src1 + so + (size_t)ix * C4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) a1[e] = __builtin_fmaf(w, v1[e], a1[e]);
          }
        }
      }
      store4<float>(dst0 + dofs + 4 * c, a0);
      if constexpr (TWO) store4<float>(dst1 + dofs + 4 * c, a1);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int launch(const char* name, const float* src0, const float* src1, const int* taps, float* dst0, float* dst1, int n_src,
           int n_dst, int C, hipStream_t s) {
  NVIT_REQUIRE(src0 && taps && dst0, "%s: NULL operand", name);
  NVIT_REQUIRE((src1 != nullptr) == (dst1 != nullptr), "%s: the second table and its result go together", name);
  NVIT_REQUIRE(n_src >= 1 && n_dst >= 1 && n_src <= NVIT_POS_RESAMPLE_MAX_GRID && n_dst <= NVIT_POS_RESAMPLE_MAX_GRID,
               "%s: grid sides %d and %d must lie in 1..%d", name, n_src, n_dst, NVIT_POS_RESAMPLE_MAX_GRID);
  NVIT_REQUIRE(n_src != n_dst, "%s: equal grids (%d) need no resampling: use the table itself", name, n_src);
  NVIT_REQUIRE(C > 0 && C % 4 == 0 && C <= NVIT_MAX_EMBD, "%s: C=%d must be a multiple of 4, at most %d", name, C,
               NVIT_MAX_EMBD);
  NVIT_REQUIRE(aligned16(src0) && aligned16(src1) && aligned16(dst0) && aligned16(dst1) && ((uintptr_t)taps & 3) == 0,
               "%s: operands must be 16-byte aligned", name);
  const long long rows = (long long)n_dst * n_dst;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, ((double)rows + (double)n_src * n_src) * C * 4.0 * (src1 ? 2.0 : 1.0), s);
  const int blocks = cdiv(rows, ROW_WAVES);
  const dim3 grid(blocks > NVIT_ROW_GRID_MAX ? NVIT_ROW_GRID_MAX : blocks), block(256);
  if (src1)
    hipLaunchKernelGGL((pos_resample_kernel<true>), grid, block, 0, s, src0, src1, taps, dst0, dst1, n_src, n_dst, C / 4);
  else
    hipLaunchKernelGGL((pos_resample_kernel<false>), grid, block, 0, s, src0, src1, taps, dst0, dst1, n_src, n_dst, C / 4);
  NVIT_CHECK_LAUNCH(name);
  return NVIT_OK;
}

}  // namespace

extern "C" int nvit_pos_resample_fwd(const float* p0, const float* p1, const int* taps, float* out0, float* out1, int g,
                                     int g2, int C, void* stream) {
  return launch("pos_resample_fwd", p0, p1, taps, out0, out1, g, g2, C, (hipStream_t)stream);
}

extern "C" int nvit_pos_resample_bwd(const float* d0, const float* d1, const int* taps_t, float* g0, float* g1, int g,
                                     int g2, int C, void* stream) {
  return launch("pos_resample_bwd", d0, d1, taps_t, g0, g1, g2, g, C, (hipStream_t)stream);
}
