// Patch dropout (timm's PatchDropout / FLIP; tests/patchdrop_ref.py is the numpy twin of the draw):
//   nvit_patchdrop_draw  one workgroup per sample -> int32 keep [B,K] (the kept tokens, ascending) and slot [B,T] (its
//                        inverse, -1 for a dropped token); a one-thread launch behind it advances the step counter
//   nvit_rows_gather     dst[b*K + j, :] = src[b*T + keep[b,j], :], one wave per kept row, float4, both streams of the
//                        embedding in one launch, optionally with their bf16 twins
//   nvit_rows_scatter    its backward: g[b*T + t, :] = d[b*K + slot[b,t], :] or zeros, one wave per destination row
// The two copies are HBM streaming kernels with the grid of the forward row kernels (rowops.hip: ROW_WAVES rows per
// workgroup, at most NVIT_ROW_GRID_MAX workgroups that stride over the rest).
#include "common.h"
#include "philox.h"

namespace {

constexpr int ROW_WAVES = NVIT_ROW_WAVES;
constexpr int PD_THREADS = 1024;   // the most threads of a draw workgroup (one per token up to here, then a stride)
constexpr int PD_MAX_T = NVIT_PATCHDROP_MAX_TOKENS;
constexpr unsigned PATCHDROP_DOMAIN = 0x50445250u;
static_assert(PD_MAX_T % 4 == 0, "the words are read four at a time");

// Token t of sample b gets the 24-bit word u = r >> 8, r = word t & 3 of the Philox call with counter (first_index + b,
// step) and the key's high word xor-ed with (domain + (t >> 2)).  Kept: the K smallest composite keys (u << 32) | t, i.e.
// a tie of u goes to the smaller t.  Rank by counting over the words in LDS (T <= 4096: T^2 compares of broadcast reads),
// then an exclusive prefix sum of the kept flags in token order gives every kept token its position.
__global__ __launch_bounds__(PD_THREADS) void patchdrop_draw_kernel(unsigned long long seed, const long long* step_ctr,
                                                                    long long first_index, int* __restrict__ keep,
                                                                    int* __restrict__ slot, int T, int K) {
  __shared__ __attribute__((aligned(16))) unsigned u[PD_MAX_T];   // the words; [T, T4) holds a sentinel above every word
  __shared__ unsigned short flag[PD_MAX_T];
  __shared__ int scan[PD_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const unsigned long long step = (unsigned long long)*step_ctr;
  const unsigned long long g = (unsigned long long)(first_index + b);
  const int T4 = (T + 3) & ~3;
  for (int q = tid; q < T4 / 4; q += nthr) {
    const Philox4 r = philox4x32_10((unsigned)g, (unsigned)(g >> 32), (unsigned)step, (unsigned)(step >> 32),
                                    (unsigned)seed, (unsigned)(seed >> 32) ^ (PATCHDROP_DOMAIN + (unsigned)q));
#pragma unroll
    for (int w = 0; w < 4; ++w) u[4 * q + w] = 4 * q + w < T ? r.v[w] >> 8 : 0xFFFFFFFFu;
  }
  __syncthreads();
  for (int t = tid; t < T; t += nthr) {
    const unsigned ut = u[t];
    int rank = 0;
    for (int j = 0; j < T4; j += 4) {   // every lane reads the same four words: one broadcast ds_read_b128
      const uint4 v = *reinterpret_cast<const uint4*>(&u[j]);
      rank += (v.x < ut || (v.x == ut && j < t)) + (v.y < ut || (v.y == ut && j + 1 < t)) +
              (v.z < ut || (v.z == ut && j + 2 < t)) + (v.w < ut || (v.w == ut && j + 3 < t));
    }
    flag[t] = rank < K;
  }
  __syncthreads();
  // prefix sum over the flags in token order: thread i owns tokens [i*per, (i+1)*per)
  const int per = (T + nthr - 1) / nthr;
  const int t0 = tid * per, t1 = min(t0 + per, T);
  int mine = 0;
  for (int t = t0; t < t1; ++t) mine += flag[t];
  scan[tid] = mine;
  __syncthreads();
  for (int o = 1; o < nthr; o <<= 1) {   // inclusive Hillis-Steele scan of the per-thread counts
    const int add = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int pos = scan[tid] - mine;
  for (int t = t0; t < t1; ++t) {
    const bool kept = flag[t];
    slot[(size_t)b * T + t] = kept ? pos : -1;
    if (kept) keep[(size_t)b * K + pos++] = t;
  }
}

// Runs behind the draw on the same stream, so every workgroup of the draw has read the counter.
__global__ void patchdrop_tick_kernel(long long* step_ctr) { *step_ctr = *step_ctr + 1; }

// One wave per kept row r = b*K + j.  An index outside [0, T) (a hand-made table) reads nothing and stores zeros.
template <bool TWO, bool LO>
__global__ __launch_bounds__(256) void rows_gather_kernel(const float* __restrict__ src0, const float* __restrict__ src1,
                                                          const int* __restrict__ keep, float* __restrict__ dst0,
                                                          float* __restrict__ dst1, bf16* __restrict__ lo0,
                                                          bf16* __restrict__ lo1, int M, int T, int K, int C4) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int r = blockIdx.x * ROW_WAVES + wid; r < M; r += gridDim.x * ROW_WAVES) {
    const int b = r / K;
    const int t = keep[r];
    const bool ok = (unsigned)t < (unsigned)T;
    const size_t so = ((size_t)b * T + (ok ? t : 0)) * C4 * 4, dofs = (size_t)r * C4 * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C4; c += 64) {
      const f32x4 v0 = ok ? load4<float>(src0 + so + 4 * c) : zero;
      f32x4 v1 = zero;
      if constexpr (TWO) v1 = ok ? load4<float>(src1 + so + 4 * c) : zero;
      store4<float>(dst0 + dofs + 4 * c, v0);
      if constexpr (LO) store4<bf16>(lo0 + dofs + 4 * c, v0);
      if constexpr (TWO) {
        store4<float>(dst1 + dofs + 4 * c, v1);
        if constexpr (LO) store4<bf16>(lo1 + dofs + 4 * c, v1);
      }
    }
  }
}

// One wave per destination row r = b*T + t: every element of g is written once, zeros where the token was dropped (or
// where a hand-made slot lies outside [0, K)).
template <bool TWO>
__global__ __launch_bounds__(256) void rows_scatter_kernel(const float* __restrict__ d0, const float* __restrict__ d1,
                                                           const int* __restrict__ slot, float* __restrict__ g0,
                                                           float* __restrict__ g1, int M, int T, int K, int C4) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int r = blockIdx.x * ROW_WAVES + wid; r < M; r += gridDim.x * ROW_WAVES) {
    const int b = r / T;
    const int j = slot[r];
    const bool ok = (unsigned)j < (unsigned)K;
    const size_t so = ((size_t)b * K + (ok ? j : 0)) * C4 * 4, dofs = (size_t)r * C4 * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C4; c += 64) {
      store4<float>(g0 + dofs + 4 * c, ok ? load4<float>(d0 + so + 4 * c) : zero);
      if constexpr (TWO) store4<float>(g1 + dofs + 4 * c, ok ? load4<float>(d1 + so + 4 * c) : zero);
    }
  }
}

int row_grid(long long M) {
  const int blocks = cdiv(M, ROW_WAVES);
  return blocks > NVIT_ROW_GRID_MAX ? NVIT_ROW_GRID_MAX : blocks;
}

bool rows_shape_ok(int B, int T, int K, int C) {
  return B > 0 && T > 0 && K > 0 && K <= T && C > 0 && C % 4 == 0 && (long long)B * T <= (1ll << 30);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int nvit_patchdrop_draw(uint64_t seed, int64_t* step, int64_t first_index, int* keep, int* slot, int B, int T,
                                   int K, void* stream) {
  NVIT_REQUIRE(step && keep && slot && first_index >= 0, "patchdrop_draw: bad arguments");
  NVIT_REQUIRE(B > 0 && T > 0 && T <= NVIT_PATCHDROP_MAX_TOKENS && K > 0 && K <= T,
               "patchdrop_draw: B=%d must be >= 1, T=%d in 1..%d, K=%d in 1..T", B, T, NVIT_PATCHDROP_MAX_TOKENS, K);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_PATCHIFY, 0.0, (double)B * (T + K) * 4.0, s);
  const int threads = T >= PD_THREADS ? PD_THREADS : ((T + 63) & ~63);   // whole waves, one thread per token where T allows
  hipLaunchKernelGGL(patchdrop_draw_kernel, dim3(B), dim3(threads), 0, s, (unsigned long long)seed, (const long long*)step,
                     (long long)first_index, keep, slot, T, K);
  NVIT_CHECK_LAUNCH("patchdrop_draw");
  hipLaunchKernelGGL(patchdrop_tick_kernel, dim3(1), dim3(1), 0, s, (long long*)step);
  NVIT_CHECK_LAUNCH("patchdrop_draw (tick)");
  return NVIT_OK;
}

extern "C" int nvit_rows_gather(const float* src0, const float* src1, const int* keep, float* dst0, float* dst1, void* lo0,
                                void* lo1, int lo_dt, int B, int T, int K, int C, void* stream) {
  NVIT_REQUIRE(src0 && keep && dst0 && rows_shape_ok(B, T, K, C),
               "rows_gather: B=%d, T=%d, K=%d (1..T), C=%d (a multiple of 4) or a NULL operand", B, T, K, C);
  NVIT_REQUIRE((src1 != nullptr) == (dst1 != nullptr), "rows_gather: src1 and dst1 go together");
  NVIT_REQUIRE(!lo0 || lo_dt == NVIT_BF16, "rows_gather: the twins are bf16");
  NVIT_REQUIRE((lo1 != nullptr) == (lo0 != nullptr && src1 != nullptr), "rows_gather: one twin per gathered stream, or none");
  NVIT_REQUIRE(aligned16(src0) && aligned16(src1) && aligned16(dst0) && aligned16(dst1) && ((uintptr_t)lo0 & 7) == 0 &&
                   ((uintptr_t)lo1 & 7) == 0, "rows_gather: operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long M = (long long)B * K;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, (double)M * C * (src1 ? 2.0 : 1.0) * (lo0 ? 10.0 : 8.0) + 4.0 * M, s);
  const dim3 grid(row_grid(M)), block(256);
  bf16 *l0 = (bf16*)lo0, *l1 = (bf16*)lo1;
  if (src1 && lo0)
    hipLaunchKernelGGL((rows_gather_kernel<true, true>), grid, block, 0, s, src0, src1, keep, dst0, dst1, l0, l1, (int)M, T, K, C / 4);
  else if (src1)
    hipLaunchKernelGGL((rows_gather_kernel<true, false>), grid, block, 0, s, src0, src1, keep, dst0, dst1, l0, l1, (int)M, T, K, C / 4);
  else if (lo0)
    hipLaunchKernelGGL((rows_gather_kernel<false, true>), grid, block, 0, s, src0, src1, keep, dst0, dst1, l0, l1, (int)M, T, K, C / 4);
  else
    hipLaunchKernelGGL((rows_gather_kernel<false, false>), grid, block, 0, s, src0, src1, keep, dst0, dst1, l0, l1, (int)M, T, K, C / 4);
  NVIT_CHECK_LAUNCH("rows_gather");
  return NVIT_OK;
}

extern "C" int nvit_rows_scatter(const float* d0, const float* d1, const int* slot, float* g0, float* g1, int B, int T,
                                 int K, int C, void* stream) {
  NVIT_REQUIRE(d0 && slot && g0 && rows_shape_ok(B, T, K, C),
               "rows_scatter: B=%d, T=%d, K=%d (1..T), C=%d (a multiple of 4) or a NULL operand", B, T, K, C);
  NVIT_REQUIRE((d1 != nullptr) == (g1 != nullptr), "rows_scatter: d1 and g1 go together");
  NVIT_REQUIRE(aligned16(d0) && aligned16(d1) && aligned16(g0) && aligned16(g1), "rows_scatter: operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const long long M = (long long)B * T;
  ProfScope ps(NVIT_KID_ROWOPS, 0.0, ((double)M * C * 4.0 + (double)B * K * C * 4.0) * (d1 ? 2.0 : 1.0) + 4.0 * M, s);
  const dim3 grid(row_grid(M)), block(256);
  if (d1)
    hipLaunchKernelGGL((rows_scatter_kernel<true>), grid, block, 0, s, d0, d1, slot, g0, g1, (int)M, T, K, C / 4);
  else
    hipLaunchKernelGGL((rows_scatter_kernel<false>), grid, block, 0, s, d0, d1, slot, g0, g1, (int)M, T, K, C / 4);
  NVIT_CHECK_LAUNCH("rows_scatter");
  return NVIT_OK;
}
