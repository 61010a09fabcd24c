// Run-time option -> compile-time argument.  Each selector calls its functor with a constant (std::integral_constant,
// usable as a template argument straight from a generic lambda's `auto` parameter) or a type tag, and returns what
// the functor returns; nested, they pick one template instantiation:
//
//   auto kernel = with_row_vecs<8>(C, [&](auto nv) {
//     return with_elem(dt, [&](auto t) { return row_kernel<nv, tag_t<decltype(t)>>; });
//   });
//
// Every branch of a selector must return the same type (a kernel pointer, or void when the functor launches itself).
#pragma once
#include <type_traits>

#include "common.h"

template <typename T>
struct type_tag {
  using type = T;
};
template <typename Tag>
using tag_t = typename Tag::type;

template <int N>
using int_c = std::integral_constant<int, N>;

// float4 vectors per lane of a 64-lane row kernel: C <= 256 * NV.  MAX_NV is the widest instantiation the family
// builds (8: C <= 2048; 16: above).
template <int MAX_NV, typename F>
static inline auto with_row_vecs(int C, F&& f) {
  static_assert(MAX_NV == 8 || MAX_NV == 16, "row kernels are built up to 8 or 16 vectors per lane");
  if (C <= 256) return f(int_c<1>{});
  if (C <= 512) return f(int_c<2>{});
  if (C <= 768) return f(int_c<3>{});
  if (C <= 1024) return f(int_c<4>{});
  if constexpr (MAX_NV == 16) {
    if (C > 2048) return f(int_c<16>{});
  }
  return f(int_c<8>{});
}

// element type of a dt: NVIT_F32 -> float, anything else -> bf16 (entry points validate dt before they dispatch)
template <typename F>
static inline auto with_elem(int dt, F&& f) {
  if (dt == NVIT_F32) return f(type_tag<float>{});
  return f(type_tag<bf16>{});
}

template <typename F>
static inline auto with_bool(bool b, F&& f) {
  if (b) return f(std::true_type{});
  return f(std::false_type{});
}

// attention head dim; the entry points have rejected anything but 32, 64 and 128
template <typename F>
static inline auto with_head_dim(int d, F&& f) {
  if (d == 32) return f(int_c<32>{});
  if (d == 64) return f(int_c<64>{});
  return f(int_c<128>{});
}

// stored head width of the head split / merge kernels; the entry points have rejected anything but 16, 32, 64 and 128
template <typename F>
static inline auto with_head_width(int dp, F&& f) {
  if (dp == 16) return f(int_c<16>{});
  return with_head_dim(dp, f);
}

// Launches through a kernel pointer that a selector returned.  The caller checks the launch (NVIT_CHECK_LAUNCH).
template <typename... P>
static inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t shmem, hipStream_t s,
                          std::common_type_t<P>... args) {
  hipLaunchKernelGGL(kernel, grid, block, shmem, s, args...);
}
