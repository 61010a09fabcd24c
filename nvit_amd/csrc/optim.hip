// Optimizer step fused with the weight re-normalisation.
//
// Replaces, for every parameter of the model, the reference's per-step sequence
//   torch.nn.utils.clip_grad_norm_(params, grad_clip)          /root/reference/nvit/train.py:935-941
//   AdamW.step()  (groups of model.py:369-385)                 /root/reference/nvit/train.py:942-944
//   Trainer.normalize_matrices()                               /root/reference/nvit/train.py:461-480, 989-990
// by two launches over a device-side parameter table:
//   grad_sqnorm_kernel : per-workgroup partial sums of ||g||^2 over all gradients (fixed order, no atomics);
//   adamw_renorm_kernel: every workgroup re-reduces those partials (same order -> same clip factor everywhere),
//                        then walks its work items: AdamW on (p, g*clip, m, v) and, for the six matrices per block
//                        that normalize_matrices touches, the row / column L2 normalisation of the UPDATED weights
//                        before they are written - each of p, g, m, v is read once and p, m, v written once
//                        (28 B per parameter; the unfused sequence moves ~52 B and needs ~20 launches).
// With skip_nonfinite (the reference's GradScaler, train.py:930-942, leaves out the step of a batch whose gradients hold
// inf or NaN) the order is grad_sqnorm, adamw_tick_guarded_kernel, adamw_renorm_kernel<const float*>: the tick sums the
// partials once, decides, and leaves a flag; the update returns before its item loop when the flag is set.
// Item kinds: -1 = plain chunk of OPT_CHUNK elements; 1 = OPT_ROWS_PER_ITEM rows, one wave per row (row norm, dim=1; cols
//             <= OPT_WIDE_COLS); 0 = slab of all rows x OPT_SLAB_COLS columns kept in LDS (column norm, dim=0), x OPT_TALL_COLS
//             above OPT_SLAB_ROWS rows (rows <= OPT_TALL_ROWS): the slab and its partial sums must fit the 160 KiB of a CU.
// AdamW arithmetic follows torch's (decoupled weight decay, bias corrections passed in from the host in double):
//   p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).
#include "common.h"

namespace {

constexpr int OPT_COLS = NVIT_OPT_TABLE_COLS;  // table columns (int64)
constexpr int OPT_CHUNK = NVIT_OPT_CHUNK;      // elements per plain item and per grad-norm chunk
constexpr int OPT_ROWS_PER_ITEM = NVIT_OPT_ROWS_PER_ITEM;  // one wave per row
constexpr int OPT_SLAB_COLS = NVIT_OPT_SLAB_COLS;  // column slab of a matrix of at most OPT_SLAB_ROWS rows
constexpr int OPT_SLAB_ROWS = NVIT_OPT_SLAB_ROWS;  //   (1152 x 32 + 128 x 32 partial sums) x 4 B = 160 KiB, all of a CU's LDS
constexpr int OPT_TALL_COLS = NVIT_OPT_TALL_COLS;  // column slab of a taller matrix
constexpr int OPT_TALL_ROWS = NVIT_OPT_TALL_ROWS;  //   (2048 x 16 + 256 x 16 partial sums) x 4 B = 144 KiB
constexpr int OPT_ROW_COLS = NVIT_OPT_ROW_COLS;    // a row of at most this many columns stays in registers (6 float4 per lane),
constexpr int OPT_WIDE_COLS = NVIT_OPT_WIDE_COLS;  //   a wider one is parked in LDS: 16 waves x 2048 x 4 B = 128 KiB
static_assert(OPT_ROWS_PER_ITEM == 1024 / 64 && OPT_ROW_COLS == 6 * 64 * 4, "a wave per row, 6 float4 per lane of it");

struct OptRow {
  float* p;
  const float* g;
  float* m;
  float* v;
  int rows, cols, kind;
  int first_item, first_chunk;
  float lr, wd;
};

__device__ __forceinline__ OptRow opt_row(const int64_t* t) {
  OptRow r;
  r.p = reinterpret_cast<float*>(t[0]);
  r.g = reinterpret_cast<const float*>(t[1]);
  r.m = reinterpret_cast<float*>(t[2]);
  r.v = reinterpret_cast<float*>(t[3]);
  r.rows = (int)t[4];
  r.cols = (int)t[5];
  r.kind = (int)t[6];
  r.first_item = (int)t[7];
  r.first_chunk = (int)t[8];
  const unsigned long long h = (unsigned long long)t[9];
  r.lr = __uint_as_float((unsigned)(h & 0xffffffffull));
  r.wd = __uint_as_float((unsigned)(h >> 32));
  return r;
}

// binary search of the table row whose [first, next first) range holds `item` (column `col` holds the firsts)
__device__ __forceinline__ int opt_find(const int64_t* table, int n, int col, int item) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)table[mid * OPT_COLS + col] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int NW>
__device__ __forceinline__ float block_sum(float s, float* red) {
  s = wave_sum(s);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = s;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += red[w];
  return t;
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const int64_t* table, int n, int total_chunks,
                                                          float* partial) {
  __shared__ float red[4];
  float s = 0.f;
  for (int item = blockIdx.x; item < total_chunks; item += gridDim.x) {
    const int mi = opt_find(table, n, 8, item);
    const OptRow r = opt_row(table + mi * OPT_COLS);
    const long long numel = (long long)r.rows * r.cols;
    const long long e0 = (long long)(item - r.first_chunk) * OPT_CHUNK;
    const long long e1 = e0 + OPT_CHUNK < numel ? e0 + OPT_CHUNK : numel;
    if ((numel & 3) == 0) {
      for (long long e = e0 + threadIdx.x * 4; e < e1; e += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(r.g + e);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
      }
    } else {
      for (long long e = e0 + threadIdx.x; e < e1; e += 256) s += r.g[e] * r.g[e];
    }
  }
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct AdamArgs {
  float b1, b2, eps, inv_bc1, inv_sqrt_bc2, max_norm;
  int npart;
};

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a, float lr, float wd,
                                      float clip) {
  g *= clip;
  p *= 1.0f - lr * wd;
  m = a.b1 * m + (1.0f - a.b1) * g;
  v = a.b2 * v + (1.0f - a.b2) * g * g;
  const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
  p -= (lr * a.inv_bc1) * (m / denom);
}

__device__ __forceinline__ void adam4(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, const AdamArgs& a, float lr,
                                      float wd, float clip) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], me = m[e], ve = v[e];
    adam1(pe, g[e], me, ve, a, lr, wd, clip);
    p[e] = pe;
    m[e] = me;
    v[e] = ve;
  }
}

// kind 0: column slab [rows][SC] of updated weights in LDS, SC = 32 columns (16 for matrices of more than OPT_SLAB_ROWS
// rows); SC / 4 threads cover the SC columns of a row, RG = 1024 / (SC / 4) row groups; the RG partial sums of a column
// are added in row-group order by one thread.  One body for both widths (the width is a shift count): two instances
// of it push the kernel over its 128 registers.
__device__ __forceinline__ void adamw_col_item(const OptRow& r, int local, int tid, float* slab, const AdamArgs& a,
                                               float clip) {
  const int sh = r.rows <= OPT_SLAB_ROWS ? 3 : 2;  // log2 of the threads across a slab row
  const int SC = 4 << sh, RG = 1024 >> sh;
  static_assert(OPT_SLAB_COLS == 4 << 3 && OPT_TALL_COLS == 4 << 2, "slab widths are 4 << sh");
  float* cred = slab + (size_t)r.rows * SC;  // [RG][SC]
  const int c0 = local * SC;
  const int cg = (tid & ((1 << sh) - 1)) * 4, rg = tid >> sh;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bool full = c0 + cg + 3 < r.cols && (r.cols & 3) == 0;
  for (int row = rg; row < r.rows; row += RG) {
    const size_t off = (size_t)row * r.cols + c0 + cg;
    f32x4 p = {0.f, 0.f, 0.f, 0.f};
    if (full) {
      p = *reinterpret_cast<const f32x4*>(r.p + off);
      const f32x4 g = *reinterpret_cast<const f32x4*>(r.g + off);
      f32x4 m = *reinterpret_cast<const f32x4*>(r.m + off);
      f32x4 v = *reinterpret_cast<const f32x4*>(r.v + off);
      adam4(p, g, m, v, a, r.lr, r.wd, clip);
      *reinterpret_cast<f32x4*>(r.m + off) = m;
      *reinterpret_cast<f32x4*>(r.v + off) = v;
    } else {
      for (int e = 0; e < 4; ++e)
        if (c0 + cg + e < r.cols) {
          float pe = r.p[off + e], me = r.m[off + e], ve = r.v[off + e];
          adam1(pe, r.g[off + e], me, ve, a, r.lr, r.wd, clip);
          r.m[off + e] = me;
          r.v[off + e] = ve;
          p[e] = pe;
        }
    }
    *reinterpret_cast<f32x4*>(slab + row * SC + cg) = p;
    acc += p * p;
  }
  *reinterpret_cast<f32x4*>(cred + rg * SC + cg) = acc;
  __syncthreads();
  if (tid < SC) {
    float s = 0.f;
    for (int gidx = 0; gidx < RG; ++gidx) s += cred[gidx * SC + tid];
    cred[tid] = sqrtf(s);  // row 0 of cred is only read by thread `tid` above before this write
  }
  __syncthreads();
  const f32x4 nrm = *reinterpret_cast<const f32x4*>(cred + cg);
  for (int row = rg; row < r.rows; row += RG) {
    const size_t off = (size_t)row * r.cols + c0 + cg;
    const f32x4 p = *reinterpret_cast<const f32x4*>(slab + row * SC + cg) / nrm;
    if (full)
      *reinterpret_cast<f32x4*>(r.p + off) = p;
    else
      for (int e = 0; e < 4; ++e)
        if (c0 + cg + e < r.cols) r.p[off + e] = p[e];
  }
  __syncthreads();
}

// 1024 threads = 16 waves, one workgroup per CU (the column slab takes most of the LDS), so the streaming items
// still have 16 waves x 4 tensors of loads in flight per CU.
// One template, two instantiations: <> is the step as it always was (same parameters, same body), <const float*> takes
// the skip state as a trailing parameter (skip_nonfinite).  There, after the norm, every workgroup reads the one flag
// that nvit_adamw_tick_guarded wrote and returns before the item loop when it is set.  The flag is a single word
// written by an earlier launch, so the decision is the same in every workgroup and thread (no workgroup updates while
// another returns), and it is taken after block_sum's barriers, with none pending.  The workgroup's own sum must NOT
// decide: the clip factor is what it is for, and a sum near FLT_MAX is finite in one order and infinite in another.
template <class... Skip>
__global__ __launch_bounds__(1024) void adamw_renorm_kernel(const int64_t* table, int n, int total_items,
                                                            const float* partial, AdamArgs a, float* gnorm_out,
                                                            const float* hyper, Skip... skip_state) {
  static_assert(sizeof...(Skip) <= 1, "at most the skip state");
  // dynamic LDS: the column slab and its partial sums (up to all 160 KiB of the CU, so nothing is declared statically);
  // its first 64 bytes serve the clip-factor sum before the item loop
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (hyper) {  // bias corrections of the device-side step counter (nvit_adamw_tick): hipGraph replays stay correct
    a.inv_bc1 = hyper[1];
    a.inv_sqrt_bc2 = hyper[2];
  }
  // global gradient norm -> clip factor (every workgroup sums the same partials in the same order)
  float clip = 1.0f;
  if (partial) {
    float s = 0.f;
    for (int i = tid; i < a.npart; i += 1024) s += partial[i];
    s = block_sum<16>(s, red);
    __syncthreads();  // `red` is the head of the slab the item loop writes
    const float nrm = sqrtf(s);
    if (a.max_norm > 0.f) {
      const float c = a.max_norm / (nrm + 1e-6f);
      clip = c < 1.0f ? c : 1.0f;
    }
    if (gnorm_out && blockIdx.x == 0 && tid == 0) gnorm_out[0] = nrm;
  }
  if constexpr (sizeof...(Skip) == 1) {
    const float* const flag[] = {skip_state...};
    if (flag[0][0] != 0.f) return;  // grid-uniform: p, m, v stay bit-identical, gnorm_out holds the inf / NaN norm
  }
  for (int item = blockIdx.x; item < total_items; item += gridDim.x) {
    const int mi = opt_find(table, n, 7, item);
    const OptRow r = opt_row(table + mi * OPT_COLS);
    const int local = item - r.first_item;
    if (r.kind < 0) {
      const long long numel = (long long)r.rows * r.cols;
      const long long e0 = (long long)local * OPT_CHUNK;
      const long long e1 = e0 + OPT_CHUNK < numel ? e0 + OPT_CHUNK : numel;
      if ((numel & 3) == 0) {
        for (long long e = e0 + tid * 4; e < e1; e += 4096) {
          f32x4 p = *reinterpret_cast<const f32x4*>(r.p + e);
          const f32x4 g = *reinterpret_cast<const f32x4*>(r.g + e);
          f32x4 m = *reinterpret_cast<const f32x4*>(r.m + e);
          f32x4 v = *reinterpret_cast<const f32x4*>(r.v + e);
          adam4(p, g, m, v, a, r.lr, r.wd, clip);
          *reinterpret_cast<f32x4*>(r.p + e) = p;
          *reinterpret_cast<f32x4*>(r.m + e) = m;
          *reinterpret_cast<f32x4*>(r.v + e) = v;
        }
      } else {
        for (long long e = e0 + tid; e < e1; e += 1024) {
          float p = r.p[e], m = r.m[e], v = r.v[e];
          adam1(p, r.g[e], m, v, a, r.lr, r.wd, clip);
          r.p[e] = p;
          r.m[e] = m;
          r.v[e] = v;
        }
      }
    } else if (r.kind == 1 && r.cols <= OPT_ROW_COLS) {
      // rows: one wave per row; the updated row stays in registers (cols <= OPT_ROW_COLS, multiple of 4) for the norm
      const int row = local * OPT_ROWS_PER_ITEM + wid;
      if (row < r.rows) {
        const size_t off = (size_t)row * r.cols;
        const int kmax = (r.cols + 255) >> 8;
        f32x4 pw[6];
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if (k < kmax) {
            const int c = (k * 64 + lane) * 4;
            const int cc = c < r.cols ? c : 0;  // clamped load, masked contribution, guarded stores
            f32x4 p = *reinterpret_cast<const f32x4*>(r.p + off + cc);
            const f32x4 g = *reinterpret_cast<const f32x4*>(r.g + off + cc);
            f32x4 m = *reinterpret_cast<const f32x4*>(r.m + off + cc);
            f32x4 v = *reinterpret_cast<const f32x4*>(r.v + off + cc);
            adam4(p, g, m, v, a, r.lr, r.wd, clip);
            if (c < r.cols) {
              *reinterpret_cast<f32x4*>(r.m + off + c) = m;
              *reinterpret_cast<f32x4*>(r.v + off + c) = v;
              ss += p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
            }
            pw[k] = p;
          }
        }
        ss = wave_sum(ss);
        const float nrm = sqrtf(ss);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int c = (k * 64 + lane) * 4;
          if (k < kmax && c < r.cols) *reinterpret_cast<f32x4*>(r.p + off + c) = pw[k] / nrm;
        }
      }
    } else if (r.kind == 1) {
      // wide rows (cols <= OPT_WIDE_COLS): 8 float4 per lane would cost the kernel its register budget, so each wave parks its
      // updated row in LDS (16 x cols x 4 B <= 128 KiB, see nvit_adamw_renorm) between the update and the scaled store
      const int row = local * OPT_ROWS_PER_ITEM + wid;
      if (row < r.rows) {
        const size_t off = (size_t)row * r.cols;
        float* prow = reinterpret_cast<float*>(smem) + wid * r.cols;
        float ss = 0.f;
        for (int c = lane * 4; c < r.cols; c += 256) {
          f32x4 p = *reinterpret_cast<const f32x4*>(r.p + off + c);
          const f32x4 g = *reinterpret_cast<const f32x4*>(r.g + off + c);
          f32x4 m = *reinterpret_cast<const f32x4*>(r.m + off + c);
          f32x4 v = *reinterpret_cast<const f32x4*>(r.v + off + c);
          adam4(p, g, m, v, a, r.lr, r.wd, clip);
          *reinterpret_cast<f32x4*>(r.m + off + c) = m;
          *reinterpret_cast<f32x4*>(r.v + off + c) = v;
          *reinterpret_cast<f32x4*>(prow + c) = p;
          ss += p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
        }
        const float nrm = sqrtf(wave_sum(ss));
        for (int c = lane * 4; c < r.cols; c += 256)  // every lane reads back what it wrote itself
          *reinterpret_cast<f32x4*>(r.p + off + c) = *reinterpret_cast<const f32x4*>(prow + c) / nrm;
      }
      __syncthreads();  // the next item may be a column slab over the same LDS
    } else {
      adamw_col_item(r, local, tid, reinterpret_cast<float*>(smem), a, clip);
    }
  }
}

// hyper[0] = step count t (after the increment), hyper[1] = 1/(1-b1^t), hyper[2] = 1/sqrt(1-b2^t)
__device__ __forceinline__ void adamw_tick(float* hyper, double b1, double b2) {
  const double t = (double)hyper[0] + 1.0;
  hyper[0] = (float)t;
  hyper[1] = (float)(1.0 / (1.0 - pow(b1, t)));
  hyper[2] = (float)(1.0 / sqrt(1.0 - pow(b2, t)));
}

__global__ void adamw_tick_kernel(float* hyper, double b1, double b2) { adamw_tick(hyper, b1, b2); }

// One workgroup: sums the norm partials (in the order adamw_renorm_kernel sums them, so the norm that kernel reports is
// non-finite exactly when the step is skipped) and takes the decision of the whole step once.  Finite: the tick, and
// skip_state[0] = 0.  Inf or NaN (a gradient holds one, or the squared norm overflows fp32): hyper stays as it is,
// skip_state[0] = 1 and skip_state[1], the count of skipped steps, goes up by one.
__global__ __launch_bounds__(1024) void adamw_tick_guarded_kernel(float* hyper, double b1, double b2,
                                                                  const float* partial, int npart, float* skip_state) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < npart; i += 1024) s += partial[i];
  s = block_sum<16>(s, red);
  if (threadIdx.x != 0) return;
  const bool finite = (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u;  // exponent all ones: inf or NaN
  if (finite) {
    adamw_tick(hyper, b1, b2);
    skip_state[0] = 0.f;
  } else {
    skip_state[0] = 1.f;
    skip_state[1] += 1.f;
  }
}

}  // namespace

extern "C" int nvit_adamw_tick(float* hyper, double beta1, double beta2, void* stream) {
  NVIT_REQUIRE(hyper && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adamw_tick: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, s, hyper, beta1, beta2);
  NVIT_CHECK_LAUNCH("adamw_tick");
  return NVIT_OK;
}

extern "C" int nvit_grad_sqnorm(const int64_t* table, int n, int total_chunks, float* partial, int npart,
                                void* stream) {
  NVIT_REQUIRE(table && partial && n > 0 && total_chunks > 0 && npart > 0 && npart <= NVIT_OPT_MAX_PART,
               "grad_sqnorm: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(NVIT_KID_OPTIM, 0.0, (double)total_chunks * OPT_CHUNK * 4.0, s);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(npart), dim3(256), 0, s, table, n, total_chunks, partial);
  NVIT_CHECK_LAUNCH("grad_sqnorm");
  return NVIT_OK;
}

// skip_state == NULL: nvit_adamw_renorm; otherwise the guarded kernel (nvit_adamw_renorm_guarded)
static int adamw_renorm_launch(const int64_t* table, int n, int total_items, int max_slab_rows, float beta1,
                               float beta2, float eps, double bias_correction1, double bias_correction2,
                               const float* partial, int npart, float max_norm, float* gnorm_out,
                               const float* hyper, const float* skip_state, void* stream) {
  NVIT_REQUIRE(table && n > 0 && total_items > 0, "adamw_renorm: empty table");
  NVIT_REQUIRE(max_slab_rows >= 0 && max_slab_rows <= OPT_TALL_ROWS,
               "adamw_renorm: column-normalised matrix with %d rows exceeds the LDS slab (%d)", max_slab_rows,
               OPT_TALL_ROWS);
  NVIT_REQUIRE(hyper || (bias_correction1 > 0.0 && bias_correction2 > 0.0),
               "adamw_renorm: bias corrections must be > 0");
  NVIT_REQUIRE(!partial || (npart > 0 && npart <= NVIT_OPT_MAX_PART), "adamw_renorm: bad npart");
  AdamArgs a;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.inv_bc1 = hyper ? 0.f : (float)(1.0 / bias_correction1);
  a.inv_sqrt_bc2 = hyper ? 0.f : (float)(1.0 / sqrt(bias_correction2));
  a.max_norm = max_norm;
  a.npart = npart;
  hipStream_t s = (hipStream_t)stream;
  // slab + [row groups][slab columns] partial sums (4096 floats in both forms).  A table whose tallest matrix takes the
  // 16-column slab may also hold one of up to OPT_SLAB_ROWS rows on the 32-column slab: size for both.  At least the 64
  // bytes of the clip-factor sum.
  static_assert(OPT_TALL_ROWS * OPT_TALL_COLS <= OPT_SLAB_ROWS * OPT_SLAB_COLS, "the tall slab fits the LDS of the wide one");
  static_assert((OPT_SLAB_ROWS * OPT_SLAB_COLS + 4096) * 4 <= 160 * 1024, "slab + partial sums fit the LDS of a CU");
  // (Rows of more than OPT_ROW_COLS columns are parked in the same LDS, 16 x cols x 4 B: the caller passes
  // max_slab_rows >= NVIT_OPT_WIDE_LDS_ROWS for a table that holds such a matrix, see nvit_hip.h.)
  static_assert(OPT_ROWS_PER_ITEM * OPT_WIDE_COLS <= NVIT_OPT_WIDE_LDS_ROWS * OPT_SLAB_COLS + 4096 &&
                NVIT_OPT_WIDE_LDS_ROWS <= OPT_SLAB_ROWS, "max_slab_rows = NVIT_OPT_WIDE_LDS_ROWS covers an item's parked rows");
  const int slab_rows = max_slab_rows > OPT_SLAB_ROWS ? OPT_SLAB_ROWS : max_slab_rows;
  const int lds = slab_rows > 0 ? (slab_rows * OPT_SLAB_COLS + 4096) * 4 : 64;
  static int lds_set[2] = {0, 0};  // per kernel
  const int which = skip_state ? 1 : 0;
  if (lds > lds_set[which]) {
    const void* fn = skip_state ? (const void*)adamw_renorm_kernel<const float*> : (const void*)adamw_renorm_kernel<>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) NVIT_FAIL((int)e, "adamw_renorm: cannot raise LDS limit: %s", hipGetErrorString(e));
    lds_set[which] = lds;
  }
  int grid = total_items < NVIT_OPT_MAX_GRID ? total_items : NVIT_OPT_MAX_GRID;
  ProfScope ps(NVIT_KID_OPTIM, 0.0, 0.0, s);
  if (skip_state)
    hipLaunchKernelGGL(adamw_renorm_kernel<const float*>, dim3(grid), dim3(1024), lds, s, table, n, total_items, partial, a,
                       gnorm_out, hyper, skip_state);
  else
    hipLaunchKernelGGL(adamw_renorm_kernel<>, dim3(grid), dim3(1024), lds, s, table, n, total_items, partial, a, gnorm_out, hyper);
  NVIT_CHECK_LAUNCH("adamw_renorm");
  return NVIT_OK;
}

extern "C" int nvit_adamw_renorm(const int64_t* table, int n, int total_items, int max_slab_rows, float beta1,
                                 float beta2, float eps, double bias_correction1, double bias_correction2,
                                 const float* partial, int npart, float max_norm, float* gnorm_out,
                                 const float* hyper, void* stream) {
  return adamw_renorm_launch(table, n, total_items, max_slab_rows, beta1, beta2, eps, bias_correction1,
                             bias_correction2, partial, npart, max_norm, gnorm_out, hyper, nullptr, stream);
}

extern "C" int nvit_adamw_tick_guarded(float* hyper, double beta1, double beta2, const float* partial, int npart,
                                       float* skip_state, void* stream) {
  NVIT_REQUIRE(hyper && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adamw_tick_guarded: bad arguments");
  NVIT_REQUIRE(partial && skip_state && npart > 0 && npart <= NVIT_OPT_MAX_PART, "adamw_tick_guarded: bad partials or skip state");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_tick_guarded_kernel, dim3(1), dim3(1024), 0, s, hyper, beta1, beta2, partial, npart,
                     skip_state);
  NVIT_CHECK_LAUNCH("adamw_tick_guarded");
  return NVIT_OK;
}

extern "C" int nvit_adamw_renorm_guarded(const int64_t* table, int n, int total_items, int max_slab_rows, float beta1,
                                         float beta2, float eps, const float* partial, int npart, float max_norm,
                                         float* gnorm_out, const float* hyper, const float* skip_state, void* stream) {
  NVIT_REQUIRE(partial && gnorm_out && hyper && skip_state,
               "adamw_renorm_guarded: needs the norm partials, gnorm_out, the device step counter and the skip state");
  return adamw_renorm_launch(table, n, total_items, max_slab_rows, beta1, beta2, eps, 0.0, 0.0, partial, npart, max_norm,
                             gnorm_out, hyper, skip_state, stream);
}

// ---- learning-rate schedule (LRSchedule) --------------------------------------------------------------------------------
// One workgroup per optimizer step, ahead of nvit_grad_sqnorm / nvit_adamw_renorm*: every thread reads the device step
// counter s and evaluates L(s) in fp64, thread 0 stores s + 1 (after a barrier: no thread may still have the load ahead
// of it), and the threads walk the table rows, storing (float)(L * lr_scale[i]) into the lr half of the row's last column.
// The weight-decay half and every other column are not touched.  L(s) is the reference trainer's get_lr
// (train.py:1025-1035) with its operation order kept, since the host restates it bit for bit
// (schedule.py): nothing from here to the end of the file contracts a multiply into an add.
#pragma clang fp contract(off)

namespace {

constexpr int LRS_THREADS = NVIT_LR_SCHEDULE_THREADS;

__global__ __launch_bounds__(LRS_THREADS) void lr_schedule_kernel(int64_t* table, int n, const float* lr_scale,
                                                                  int64_t* step, int kind, double lr, double min_lr,
                                                                  double warmup_init, int64_t W, int64_t D,
                                                                  float* last_lr, double* last_lr64) {
  const int64_t s = step[0];
  double L;
  if (s < W) {
    L = warmup_init + (lr - warmup_init) * (double)s / (double)W;
  } else if (kind == NVIT_LR_CONSTANT) {
    L = lr;
  } else if (s > D) {
    L = min_lr;
  } else {
    const double r = (double)(s - W) / (double)(D - W);
    if (kind == NVIT_LR_COSINE)
      L = min_lr + (0.5 * (1.0 + cos(3.141592653589793 * r))) * (lr - min_lr);
    else
      L = lr + (min_lr - lr) * r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    step[0] = s + 1;
    last_lr[0] = (float)L;
    last_lr64[0] = L;
  }
  for (int i = threadIdx.x; i < n; i += LRS_THREADS) {
    const float v = (float)(L * (double)lr_scale[i]);
    // the low word of the little-endian int64 {f32bits(lr) | f32bits(weight_decay) << 32}
    reinterpret_cast<float*>(table + (size_t)i * OPT_COLS + (OPT_COLS - 1))[0] = v;
  }
}

}  // namespace

extern "C" int nvit_lr_schedule(int64_t* table, int n, const float* lr_scale, int64_t* step, int kind, double lr,
                                double min_lr, double warmup_init, int64_t warmup_iters, int64_t decay_iters,
                                float* last_lr, double* last_lr64, void* stream) {
  NVIT_REQUIRE(step && last_lr && last_lr64 && n >= 0 && (n == 0 || (table && lr_scale)), "lr_schedule: bad arguments");
  NVIT_REQUIRE(kind == NVIT_LR_COSINE || kind == NVIT_LR_LINEAR || kind == NVIT_LR_CONSTANT, "lr_schedule: unknown kind %d",
               kind);
  NVIT_REQUIRE(warmup_iters >= 0 && (kind == NVIT_LR_CONSTANT || decay_iters > warmup_iters),
               "lr_schedule: needs warmup_iters >= 0 and decay_iters > warmup_iters");
  NVIT_REQUIRE(lr >= 0.0 && min_lr >= 0.0 && warmup_init >= 0.0 && lr <= 1.79e308 && min_lr <= 1.79e308 &&
               warmup_init <= 1.79e308, "lr_schedule: rates must be finite and >= 0");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(LRS_THREADS), 0, s, table, n, lr_scale, step, kind, lr, min_lr,
                     warmup_init, warmup_iters, decay_iters, last_lr, last_lr64);
  NVIT_CHECK_LAUNCH("lr_schedule");
  return NVIT_OK;
}
