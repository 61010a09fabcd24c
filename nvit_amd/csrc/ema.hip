// Exponential moving average of the weights (timm's ModelEmaV2 / `--model-ema` of the DeiT recipe) as two launches over
// a device-side table, so that it is captured with the train step and replayed without host work:
//   ema_tick_kernel  : one thread; advances the update count and leaves omd = 1 - decay(t) for the update about to run,
//                      or omd = 0 when the optimizer's guarded tick left this step out (skip_nonfinite);
//   ema_update_kernel: every workgroup reads that one word, written by the earlier launch, and returns before it touches
//                      memory when it is 0; otherwise it walks fixed-size chunks of the table's rows:
//                      e = fma(omd, p - e, e), or e = p for a row flagged "copy" (e + 1 * (p - e) is not p in floating
//                      point, so a copy is its own branch and not omd = 1).
// 12 B per element (p and e read, e written), float4 accesses; a row whose length is no multiple of 4 or whose pointers
// are not 16-byte aligned carries NVIT_EMA_FLAG_SCALAR (set by the host, the kernel does not guess) and runs element by
// element.  src and dst ranges must not overlap: the host wrapper refuses such a table.
#include "common.h"

namespace {

constexpr int EMA_COLS = NVIT_EMA_TABLE_COLS;
constexpr int EMA_CHUNK = NVIT_EMA_CHUNK;
static_assert(EMA_CHUNK % 1024 == 0, "a chunk is whole passes of 256 threads x float4");

// state[0] = t, the updates applied so far (exact up to 2^24, like the optimizer's hyper[0]); state[1] = omd
__global__ void ema_tick_kernel(float* state, double decay, int warmup, const float* skip_state) {
  if (skip_state && skip_state[0] != 0.f) {  // the optimizer step was left out: so is this update, the count stays
    state[1] = 0.f;
    return;
  }
  const double t = (double)state[0];
  double d = decay;
  if (warmup) {
    const double w = (1.0 + t) / (10.0 + t);
    d = w < d ? w : d;
  }
  state[1] = (float)(1.0 - d);
  state[0] = (float)(t + 1.0);
}

// binary search of the table row whose [first_chunk, next first_chunk) range holds `item`
__device__ __forceinline__ int ema_find(const int64_t* table, int n, int item) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)table[mid * EMA_COLS + 3] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// state == nullptr: only the copy rows run (ModelEma.sync), the others are left alone.
__global__ __launch_bounds__(256) void ema_update_kernel(const int64_t* table, int n, int total_chunks,
                                                         const float* state) {
  float omd = 0.f;
  if (state) {
    omd = state[1];
    if (omd == 0.f) return;  // grid-uniform (one word of an earlier launch): a skipped step leaves every bit in place
  }
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < total_chunks; item += gridDim.x) {
    const int64_t* row = table + (size_t)ema_find(table, n, item) * EMA_COLS;
    const float* src = reinterpret_cast<const float*>(row[0]);
    float* dst = reinterpret_cast<float*>(row[1]);
    const long long numel = row[2];
    const int flags = (int)row[4];
    const bool copy = (flags & NVIT_EMA_FLAG_COPY) != 0;
    if (!copy && !state) continue;
    const long long e0 = (long long)(item - (int)row[3]) * EMA_CHUNK;
    const long long e1 = e0 + EMA_CHUNK < numel ? e0 + EMA_CHUNK : numel;
    if (!(flags & NVIT_EMA_FLAG_SCALAR) && e1 - e0 == EMA_CHUNK) {
      // a whole chunk (all but the last of a row): every load of the thread is issued before the first store
      constexpr int PASSES = EMA_CHUNK / 1024;
      const float* s = src + e0 + tid * 4;
      float* d = dst + e0 + tid * 4;
      f32x4 p[PASSES], e[PASSES];
#pragma unroll
      for (int k = 0; k < PASSES; ++k) p[k] = *reinterpret_cast<const f32x4*>(s + k * 1024);
      if (!copy) {
#pragma unroll
        for (int k = 0; k < PASSES; ++k) e[k] = *reinterpret_cast<const f32x4*>(d + k * 1024);
#pragma unroll
        for (int k = 0; k < PASSES; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) p[k][j] = __builtin_fmaf(omd, p[k][j] - e[k][j], e[k][j]);
      }
#pragma unroll
      for (int k = 0; k < PASSES; ++k) *reinterpret_cast<f32x4*>(d + k * 1024) = p[k];
    } else if (!(flags & NVIT_EMA_FLAG_SCALAR)) {
      for (long long i = e0 + tid * 4; i < e1; i += 1024) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(src + i);
        if (copy) {
          *reinterpret_cast<f32x4*>(dst + i) = p;
        } else {
          f32x4 e = *reinterpret_cast<const f32x4*>(dst + i);
#pragma unroll
          for (int k = 0; k < 4; ++k) e[k] = __builtin_fmaf(omd, p[k] - e[k], e[k]);
          *reinterpret_cast<f32x4*>(dst + i) = e;
        }
      }
    } else {
      for (long long i = e0 + tid; i < e1; i += 256) {
        const float p = src[i];
        dst[i] = copy ? p : __builtin_fmaf(omd, p - dst[i], dst[i]);
      }
    }
  }
}

}  // namespace

extern "C" int nvit_ema_tick(float* state, double decay, int warmup, const float* skip_state, void* stream) {
  NVIT_REQUIRE(state && decay >= 0.0 && decay < 1.0, "ema_tick: needs the state and a decay in [0, 1)");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(1), 0, s, state, decay, warmup, skip_state);
  NVIT_CHECK_LAUNCH("ema_tick");
  return NVIT_OK;
}

extern "C" int nvit_ema_update(const int64_t* table, int n, int total_chunks, const float* state, void* stream) {
  NVIT_REQUIRE(table && n > 0 && total_chunks > 0, "ema_update: empty table");
  hipStream_t s = (hipStream_t)stream;
  const int grid = total_chunks < NVIT_EMA_MAX_GRID ? total_chunks : NVIT_EMA_MAX_GRID;
  ProfScope ps(NVIT_KID_OPTIM, 0.0, (double)total_chunks * EMA_CHUNK * 12.0, s);
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(256), 0, s, table, n, total_chunks, state);
  NVIT_CHECK_LAUNCH("ema_update");
  return NVIT_OK;
}
