// Device-resident dataset ("The device-resident dataset"; tests/loader_ref.py is the numpy twin of the draw):
//   nvit_loader_draw    ONE workgroup -> int64 idx [B], the images of this rank's batch at step *step, and the record
//                       {epoch, step in the epoch}; every thread reads the counter, a barrier, then thread 0 stores
//                       counter + 1: no tick launch behind it
//   nvit_loader_gather  out[b] = images[idx[b]] (rows of row_bytes bytes, 64-bit offsets) and y[b] = labels[idx[b]]; work
//                       items (image, chunk of GATHER_CHUNK bytes), 16 bytes per lane where row size and both bases allow
//                       it, single bytes otherwise
// The gather is an HBM streaming copy: at most GATHER_GRID_MAX workgroups that stride over the work items.
#include "common.h"
#include "philox.h"

namespace {

constexpr int DRAW_THREADS = 1024;
constexpr unsigned LOADER_DOMAIN = 0x4C4F4144u;
constexpr int FEISTEL_ROUNDS = 4;
constexpr int GATHER_THREADS = 256;
constexpr int GATHER_CHUNK = GATHER_THREADS * 16;   // bytes of a row that one workgroup copies at a time
constexpr int GATHER_GRID_MAX = 4096;

// perm_{seed,epoch}(x) of [0, N): a balanced Feistel network on 2 * half bits, re-applied while the value is >= N (cycle
// walking: the network permutes [0, 4^half) and the walk starts inside [0, N), so it comes back there).
__device__ __forceinline__ unsigned long long loader_perm(unsigned long long x, unsigned long long N, int half,
                                                         unsigned long long epoch, unsigned k0, unsigned k1) {
  const unsigned mask = (unsigned)((1ull << half) - 1ull);
  do {
    unsigned L = (unsigned)(x >> half), R = (unsigned)x & mask;
#pragma unroll
    for (int j = 0; j < FEISTEL_ROUNDS; ++j) {
      const Philox4 r = philox4x32_10(R, (unsigned)j, (unsigned)epoch, (unsigned)(epoch >> 32), k0, k1);
      const unsigned n = L ^ (r.v[0] & mask);
      L = R;
      R = n;
    }
    x = ((unsigned long long)L << half) | R;
  } while (x >= N);
  return x;
}

__global__ __launch_bounds__(DRAW_THREADS) void loader_draw_kernel(unsigned long long seed, long long* step_ctr,
                                                                   unsigned long long N, unsigned long long S,
                                                                   unsigned long long G, unsigned long long first_row,
                                                                   unsigned long long repeats, int shuffle, int half,
                                                                   long long* __restrict__ idx, long long* __restrict__ record,
                                                                   int B) {
  const unsigned long long s = (unsigned long long)*step_ctr;
  const unsigned long long epoch = s / S, t = s % S;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ LOADER_DOMAIN;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const unsigned long long p = (t * G + first_row + (unsigned long long)i) / repeats;   // < N: S * G <= N * repeats
    idx[i] = (long long)(shuffle ? loader_perm(p, N, half, epoch, k0, k1) : p);
  }
  __syncthreads();   // every thread of the one workgroup has read the counter
  if (threadIdx.x == 0) {
    record[0] = (long long)epoch;
    record[1] = (long long)t;
    *step_ctr = (long long)(s + 1ull);
  }
}

// Work item w = (image b, chunk c).  An index outside [0, N) (a hand-made table) reads nothing: zeros, label 0.
template <bool VEC>
__global__ __launch_bounds__(GATHER_THREADS) void loader_gather_kernel(const unsigned char* __restrict__ images,
                                                                       const long long* __restrict__ labels,
                                                                       const long long* __restrict__ idx,
                                                                       unsigned char* __restrict__ out,
                                                                       long long* __restrict__ y, long long N,
                                                                       long long row_bytes, int chunks, long long items) {
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const long long b = w / chunks;
    const long long c0 = (w - b * chunks) * GATHER_CHUNK;
    const long long n = idx[b];
    const bool ok = n >= 0 && n < N;
    const unsigned char* src = images + (ok ? n : 0) * row_bytes;
    unsigned char* dst = out + b * row_bytes;
    if (c0 == 0 && threadIdx.x == 0) y[b] = ok ? labels[n] : 0;
    if constexpr (VEC) {
      const long long o = c0 + (long long)threadIdx.x * 16;
      if (o < row_bytes) {   // row_bytes % 16 == 0: a whole vector or none
        uint4 v = {0u, 0u, 0u, 0u};
        if (ok) v = *reinterpret_cast<const uint4*>(src + o);
        *reinterpret_cast<uint4*>(dst + o) = v;
      }
    } else {
      const long long end = c0 + GATHER_CHUNK < row_bytes ? c0 + GATHER_CHUNK : row_bytes;
      for (long long o = c0 + threadIdx.x; o < end; o += GATHER_THREADS) dst[o] = ok ? src[o] : (unsigned char)0;
    }
  }
}

}  // namespace

extern "C" int nvit_loader_draw(uint64_t seed, int64_t* step, int64_t N, int64_t steps_per_epoch, int64_t global_batch,
                                int64_t first_row, int repeats, int shuffle, int64_t* idx, int64_t* record, int B,
                                void* stream) {
  NVIT_REQUIRE(step && idx && record, "loader_draw: NULL operand");
  NVIT_REQUIRE(N >= 1 && N <= NVIT_LOADER_MAX_IMAGES && B >= 1 && B <= NVIT_LOADER_MAX_BATCH && repeats >= 1 &&
                   repeats <= NVIT_LOADER_MAX_REPEATS,   // N * repeats, the positions of an epoch, stays far inside 64 bits
               "loader_draw: N=%lld in 1..2^40, B=%d in 1..%d, repeats=%d in 1..%d", (long long)N, B, NVIT_LOADER_MAX_BATCH,
               repeats, NVIT_LOADER_MAX_REPEATS);
  NVIT_REQUIRE(global_batch >= B && first_row >= 0 && first_row + B <= global_batch && global_batch <= (1ll << 40),
               "loader_draw: rows [%lld, %lld + %d) must lie in the global batch of %lld", (long long)first_row,
               (long long)first_row, B, (long long)global_batch);
  // every position of an epoch maps into [0, N): (S * G - 1) / repeats < N
  NVIT_REQUIRE(steps_per_epoch >= 1 && steps_per_epoch <= (N * (int64_t)repeats) / global_batch,
               "loader_draw: steps_per_epoch=%lld must be 1..(N * repeats) / global_batch", (long long)steps_per_epoch);
  int w = 2;
  while (w < 62 && (1ll << w) < N) w += 2;   // the smallest even number of bits that holds N - 1, at least 2
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_MISC, 0.0, (double)B * 8.0, s);
  const int threads = B >= DRAW_THREADS ? DRAW_THREADS : ((B + 63) & ~63);
  hipLaunchKernelGGL(loader_draw_kernel, dim3(1), dim3(threads), 0, s, (unsigned long long)seed, (long long*)step,
                     (unsigned long long)N, (unsigned long long)steps_per_epoch, (unsigned long long)global_batch,
                     (unsigned long long)first_row, (unsigned long long)repeats, shuffle ? 1 : 0, w / 2, (long long*)idx,
                     (long long*)record, B);
  NVIT_CHECK_LAUNCH("loader_draw");
  return NVIT_OK;
}

extern "C" int nvit_loader_gather(const void* images, const int64_t* labels, const int64_t* idx, void* out, int64_t* y,
                                  int64_t N, int64_t row_bytes, int B, void* stream) {
  NVIT_REQUIRE(images && labels && idx && out && y, "loader_gather: NULL operand");
  NVIT_REQUIRE(N >= 1 && N <= NVIT_LOADER_MAX_IMAGES && B >= 1 && B <= NVIT_LOADER_MAX_BATCH && row_bytes >= 1 &&
                   row_bytes <= (1ll << 31),
               "loader_gather: N=%lld in 1..2^40, B=%d in 1..%d, row_bytes=%lld in 1..2^31", (long long)N, B,
               NVIT_LOADER_MAX_BATCH, (long long)row_bytes);
  hipStream_t s = (hipStream_t)stream;
  const int chunks = cdiv(row_bytes, GATHER_CHUNK);
  const long long items = (long long)B * chunks;
  ProfScope ps(NVIT_KID_MISC, 0.0, 2.0 * (double)B * (double)row_bytes + 24.0 * B, s);
  const dim3 grid((unsigned)(items > GATHER_GRID_MAX ? GATHER_GRID_MAX : items)), block(GATHER_THREADS);
  const bool vec = row_bytes % 16 == 0 && ((uintptr_t)images & 15) == 0 && ((uintptr_t)out & 15) == 0;
  const unsigned char* im = (const unsigned char*)images;
  if (vec)
    hipLaunchKernelGGL((loader_gather_kernel<true>), grid, block, 0, s, im, (const long long*)labels, (const long long*)idx,
                       (unsigned char*)out, (long long*)y, (long long)N, (long long)row_bytes, chunks, items);
  else
    hipLaunchKernelGGL((loader_gather_kernel<false>), grid, block, 0, s, im, (const long long*)labels, (const long long*)idx,
                       (unsigned char*)out, (long long*)y, (long long)N, (long long)row_bytes, chunks, items);
  NVIT_CHECK_LAUNCH("loader_gather");
  return NVIT_OK;
}
