// MIN / MAX over window frames given as inclusive row ranges [s_i, t_i], for
// MI355X (gfx950): a range-min query per output row, so the frames of a ROWS
// or RANGE window (any offsets, any partitioning, monotone or not) cost the
// same few loads per row whatever their length.
//
// Values become order-preserving uint64 keys at load and are turned back at
// store: int64 takes x ^ sign bit, float64 the transform of grouped_select.hip
// (negatives: all bits flipped, otherwise the sign bit flipped; every NaN
// takes the all-ones key, so NaN is the largest value and -0.0 sorts below
// +0.0). An invalid row enters as the operation's identity: all ones for min,
// zero for max.
//
// Rows are cut into blocks of 64, one wavefront per block.
//
//  wf_block_scan   (four blocks per 256-thread workgroup) loads x and valid
//        coalesced, makes the key, takes an inclusive prefix op over
//        __shfl_up and an inclusive suffix op over __shfl_down, six steps
//        each, and writes P[i] = op(block start .. i), S[i] = op(i .. block
//        end) and the block's aggregate to level 0 of a table over blocks.
//        The tail block pads with the identity.
//  wf_sparse_level (one launch per level) level k of a sparse table over the
//        nb = ceil(n / 64) block aggregates: L_k[j] = op(L_{k-1}[j],
//        L_{k-1}[j + 2^(k-1)]) for every j with j + 2^k <= nb.
//  wf_query        one lane per output row, s and t read coalesced. Frames
//        that span blocks take op(S[s], P[t]) and, with m = bt - bs - 1 >= 1
//        whole blocks between, L_k[bs + 1] and L_k[bt - 2^k] for
//        k = floor(log2(m)): four loads that do not depend on each other. A
//        frame inside one block is P[t] when it starts the block, S[s] when it
//        ends it, and otherwise a loop over its at most 62 rows of x and
//        valid, which are the neighbouring lanes' cache lines.
//
// No kernel waits for another workgroup: the passes are separate launches.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cstdint>

namespace {

constexpr int kBlock = 256;   // threads per workgroup
constexpr int kShift = 6;     // rows per block = one wavefront
constexpr int kRows = 1 << kShift;
constexpr unsigned long long kSign = 1ull << 63;

using u64 = unsigned long long;

template <typename T>
__device__ inline u64 to_key(T v);
template <>
__device__ inline u64 to_key<int64_t>(int64_t v) {
  return (u64)v ^ kSign;
}
template <>
__device__ inline u64 to_key<double>(double v) {
  if (v != v) return ~0ull;
  const u64 b = (u64)__double_as_longlong(v);
  return (b & kSign) ? ~b : (b | kSign);
}

template <typename T>
__device__ inline T from_key(u64 k);
template <>
__device__ inline int64_t from_key<int64_t>(u64 k) {
  return (int64_t)(k ^ kSign);
}
template <>
__device__ inline double from_key<double>(u64 k) {  // the all-ones key gives a NaN
  return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k));
}

template <bool MAX>
__device__ inline u64 comb(u64 a, u64 b) {
  if constexpr (MAX) return a > b ? a : b;
  else return a < b ? a : b;
}

template <bool MAX>
constexpr u64 kIdentity = MAX ? 0ull : ~0ull;

template <typename T, bool MAX>
__global__ __launch_bounds__(kBlock) void wf_block_scan(
    const T* __restrict__ x, const uint8_t* __restrict__ valid, int64_t n, int64_t nb,
    u64* __restrict__ P, u64* __restrict__ S, u64* __restrict__ L0) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kRows - 1);
  u64 key = kIdentity<MAX>;
  if (i < n && (!valid || valid[i])) key = to_key<T>(x[i]);
  // every lane of the wave reaches every shuffle: nothing has returned yet
  u64 p = key, s = key;
#pragma unroll
  for (int d = 1; d < kRows; d <<= 1) {
    const u64 up = __shfl_up(p, d, kRows);
    const u64 down = __shfl_down(s, d, kRows);
    if (lane >= d) p = comb<MAX>(p, up);
    if (lane + d < kRows) s = comb<MAX>(s, down);
  }
  if (i < n) {
    P[i] = p;
    S[i] = s;
  }
  const int64_t blk = i >> kShift;
  if (lane == kRows - 1 && blk < nb) L0[blk] = p;
}

// cur[j] = op(prev[j], prev[j + half]) for j < count, where count = nb - 2 * half + 1
template <bool MAX>
__global__ __launch_bounds__(kBlock) void wf_sparse_level(const u64* __restrict__ prev,
                                                          u64* __restrict__ cur, int64_t half,
                                                          int64_t count) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < count) cur[j] = comb<MAX>(prev[j], prev[j + half]);
}

template <typename T, bool MAX>
__global__ __launch_bounds__(kBlock) void wf_query(
    const T* __restrict__ x, const uint8_t* __restrict__ valid, const int64_t* __restrict__ s_pos,
    const int64_t* __restrict__ t_pos, const u64* __restrict__ P, const u64* __restrict__ S,
    const u64* __restrict__ L, int64_t n, int64_t nb, int top, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int64_t s = s_pos[i], t = t_pos[i];
  // the contract keeps a frame inside [0, n); the clamps keep every load there
  // for input that breaks it
  s = s < 0 ? 0 : s;
  t = t >= n ? n - 1 : t;
  if (s > t) {
    out[i] = T(0);
    return;
  }
  const int64_t bs = s >> kShift, bt = t >> kShift;
  u64 r;
  if (bs != bt) {
    r = comb<MAX>(S[s], P[t]);
    const int64_t m = bt - bs - 1;
    if (m >= 1) {
      const int k = 63 - __clzll((long long)m);
      if (k <= top) {
        const u64* lv = L + (int64_t)k * nb;
        r = comb<MAX>(r, comb<MAX>(lv[bs + 1], lv[bt - ((int64_t)1 << k)]));
      } else {
        // a frame longer than the bound the table was built for: walk the top level
        const u64* lv = L + (int64_t)top * nb;
        const int64_t w = (int64_t)1 << top;
        for (int64_t j = bs + 1; j + w <= bt; j += w) r = comb<MAX>(r, lv[j]);
        r = comb<MAX>(r, lv[bt - w]);
      }
    }
  } else if ((s & (kRows - 1)) == 0) {
    r = P[t];
  } else if ((t & (kRows - 1)) == kRows - 1 || t == n - 1) {
    r = S[s];
  } else {
    r = kIdentity<MAX>;
    for (int64_t j = s; j <= t; ++j)
      if (!valid || valid[j]) r = comb<MAX>(r, to_key<T>(x[j]));
  }
  out[i] = from_key<T>(r);
}

template <typename T, bool MAX>
void launch_all(const torch::Tensor& x, const uint8_t* valid, const torch::Tensor& s_pos,
                const torch::Tensor& t_pos, u64* P, u64* S, u64* L, int64_t n, int64_t nb, int top,
                torch::Tensor& out, hipStream_t stream) {
  const T* xp = (const T*)x.data_ptr();
  const int grid = (int)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((wf_block_scan<T, MAX>), dim3(grid), dim3(kBlock), 0, stream, xp, valid, n, nb,
                     P, S, L);
  for (int k = 1; k <= top; ++k) {
    const int64_t half = (int64_t)1 << (k - 1);
    const int64_t count = nb - 2 * half + 1;   // >= 1: 2^top <= nb - 2
    hipLaunchKernelGGL((wf_sparse_level<MAX>), dim3((int)((count + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, stream, L + (int64_t)(k - 1) * nb, L + (int64_t)k * nb,
                       half, count);
  }
  hipLaunchKernelGGL((wf_query<T, MAX>), dim3(grid), dim3(kBlock), 0, stream, xp, valid,
                     s_pos.data_ptr<int64_t>(), t_pos.data_ptr<int64_t>(), P, S, L, n, nb, top,
                     (T*)out.data_ptr());
}

}  // namespace

// out[i] = min (op 0) or max (op 1) of the valid x[s_pos[i] .. t_pos[i]], both
// ends inclusive, in Spark's order (NaN largest, -0.0 below +0.0). x is int64
// or float64 with rows in window order; valid is uint8 or bool, or absent.
// Where s <= t the caller keeps 0 <= s and t < n; s > t is an empty frame and
// stores 0. A frame without a valid row stores an unspecified value: the
// caller masks it. The frames need not be monotone. max_frame_rows > 0 is the
// caller's bound on t - s + 1: the table over blocks then stops at the level
// such frames reach (longer frames stay right, they walk the top level);
// 0 builds every level. Extra memory: 16 B per row for P and S, plus
// 8 * ceil(n / 64) * (levels + 1) for the table. Launches on the tensors'
// device and the current stream; never synchronises; n == 0 launches nothing.
torch::Tensor window_frame_minmax(torch::Tensor x, c10::optional<torch::Tensor> valid,
                                  torch::Tensor s_pos, torch::Tensor t_pos, int64_t op,
                                  int64_t max_frame_rows) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 1 &&
                  (x.scalar_type() == torch::kInt64 || x.scalar_type() == torch::kFloat64),
              "window_frame_minmax: x must be a contiguous cuda int64 or float64 vector");
  const int64_t n = x.numel();
  TORCH_CHECK(n < (int64_t(1) << 37), "window_frame_minmax: fewer than 2^37 rows");
  TORCH_CHECK(op == 0 || op == 1, "window_frame_minmax: op is 0 (min) or 1 (max)");
  TORCH_CHECK(max_frame_rows >= 0, "window_frame_minmax: max_frame_rows must not be negative");
  for (const torch::Tensor* p : {&s_pos, &t_pos})
    TORCH_CHECK(p->is_cuda() && p->is_contiguous() && p->dim() == 1 && p->numel() == n &&
                    p->device() == x.device() && p->scalar_type() == torch::kInt64,
                "window_frame_minmax: s_pos and t_pos must be contiguous cuda int64 vectors of "
                "x's length on x's device");
  const uint8_t* vptr = nullptr;
  if (valid.has_value() && valid->defined()) {
    TORCH_CHECK(valid->scalar_type() == torch::kUInt8 || valid->scalar_type() == torch::kBool,
                "window_frame_minmax: valid must be uint8 or bool");
    TORCH_CHECK(valid->is_cuda() && valid->is_contiguous() && valid->numel() == n &&
                    valid->device() == x.device(),
                "window_frame_minmax: valid must be a contiguous cuda tensor of x's length on "
                "x's device");
    vptr = (const uint8_t*)valid->data_ptr();
  }

  c10::DeviceGuard guard(x.device());
  auto out = torch::empty_like(x);
  if (n == 0) return out;
  const int64_t nb = (n + kRows - 1) >> kShift;
  // the most whole blocks between the two ends of a frame: s on the last row
  // of its block and t on the first of its own give t - s + 1 = 64 m + 2
  int64_t m_max = nb - 2;
  if (max_frame_rows > 0) m_max = std::min<int64_t>(m_max, (max_frame_rows - 2) / kRows);
  int top = 0;   // floor(log2(m_max)), 0 below 2
  while ((int64_t(2) << top) <= m_max) ++top;
  // everything is allocated before the first launch below; every entry a
  // query reads is written by a launch before it
  const auto i64 = x.options().dtype(torch::kInt64);
  auto ps = torch::empty({2, n}, i64);
  auto table = torch::empty({top + 1, nb}, i64);
  u64* P = (u64*)ps.data_ptr<int64_t>();
  u64* L = (u64*)table.data_ptr<int64_t>();
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const bool f64 = x.scalar_type() == torch::kFloat64;
  if (f64 && op) launch_all<double, true>(x, vptr, s_pos, t_pos, P, P + n, L, n, nb, top, out, stream);
  else if (f64) launch_all<double, false>(x, vptr, s_pos, t_pos, P, P + n, L, n, nb, top, out, stream);
  else if (op) launch_all<int64_t, true>(x, vptr, s_pos, t_pos, P, P + n, L, n, nb, top, out, stream);
  else launch_all<int64_t, false>(x, vptr, s_pos, t_pos, P, P + n, L, n, nb, top, out, stream);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "window_frame_minmax launch failed: ", hipGetErrorString(e));
  return out;
}
