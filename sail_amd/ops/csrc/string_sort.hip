// Ordering kernels for raw string columns on MI355X (gfx950).
//
// Arrow-layout strings (offsets int64[n+1], bytes uint8[total]) in unsigned
// byte-lexicographic order, a proper prefix first ("a" < "a\0" < "b"):
//   str_sort_perm   — stable argsort of the column, or of a subset of its rows
//   str_dense_rank  — dense ranks along a sorted permutation
//   str_compare3    — row-wise three-way compare of two columns, or of a
//                     column and one broadcast value
//
// The sort is a merge sort over (key, index) pairs, 12 B per row:
//   key   uint64: the first 8 bytes, big-endian, zero padded, so one unsigned
//         compare orders 8 bytes
//   index uint32: the position in `rows` (m < 2^32), also the tie-break that
//         makes the order total, hence the result unique and stable
// Keys that differ decide a comparison; equal keys with a length <= 8 on
// either side are decided by the lengths (the shorter one is a prefix of the
// other); only otherwise are the bytes read, from byte 8 on, 8 per step.
//
//  - tile sort: a workgroup of 256 threads owns 2048 pairs in LDS (16 KB of
//    keys + 8 KB of indices, 6 workgroups per CU by LDS). Each thread sorts its
//    8 consecutive pairs in registers (Batcher's 19-comparator network), then
//    8 merge rounds run in LDS: a thread finds its 8 outputs by a merge-path
//    binary search over the two runs it straddles, merges them serially into
//    registers, and after a barrier writes them back. The tile leaves with
//    coalesced stores.
//  - global passes: ceil(log2(tiles)) passes between two (key, index) buffers.
//    A partition kernel places one merge-path diagonal per 2048 outputs; the
//    merge kernel loads the <= 2048 inputs of its output tile into LDS and
//    merges as above. A last run without a partner is an empty-B merge, a copy.
//    A pass moves 24 B per row.
//
// One deviation from a separate key pass: the keys are built by the tile
// sort's own coalesced load (one thread per row, same code), which saves
// writing and re-reading 12 B per row.
//
// Bytes are read as the aligned dwords around the source, funnel-shifted and
// byte-swapped; a dword that would reach past bytes.numel() is assembled from
// its bytes, so nothing at or past the end is read. Offsets are engine-made
// and trusted (monotone, inside `bytes`), as like_mask trusts them; `rows`
// values are not range-checked, since that would cost a synchronisation.
//
// Known slow case: many long equal strings. Every comparison between them
// walks the whole value, so the sort costs O(len) per comparison there.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstdint>
#include <vector>

#define SAIL_CHECK(x) TORCH_CHECK(x, #x)
// launches go to the tensors' device, whichever is current
#define SAIL_DEVICE_GUARD(t) \
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA device_guard(t.device())

namespace {

constexpr int kBlock = 256;
constexpr int kPer = 8;
constexpr int kTile = kBlock * kPer;  // 2048 pairs, 24 KB of LDS
constexpr uint32_t kPadIndex = 0xffffffffu;  // m < 2^32, so never a position

inline int grid_for(int64_t n) {
  int64_t blocks = (n + kBlock - 1) / kBlock;
  return (int)std::min<int64_t>(blocks, 2048);
}

// a column as the comparator sees it
struct StrView {
  const int64_t* offsets;
  const uint8_t* bytes;  // 4-byte aligned
  int64_t nbytes;
  const int64_t* rows;   // sorted subset, or null for all rows
  uint32_t m;            // pairs with index >= m are padding
};

__device__ __forceinline__ uint32_t load_dword(const uint8_t* bytes, int64_t nbytes,
                                               int64_t q) {
  if (q + 4 <= nbytes) return *reinterpret_cast<const uint32_t*>(bytes + q);
  uint32_t v = 0;  // the last, partial dword of the buffer
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (q + k < nbytes) v |= (uint32_t)bytes[q + k] << (8 * k);
  return v;
}

// bytes[pos, pos + avail) as a big-endian word, zero padded; 1 <= avail <= 8
__device__ __forceinline__ uint64_t load_be64(const uint8_t* bytes, int64_t nbytes,
                                              int64_t pos, int avail) {
  int64_t p = pos & ~(int64_t)3;
  int sh = (int)(pos & 3) * 8;
  int64_t end = pos + avail;
  uint64_t lo = load_dword(bytes, nbytes, p);
  if (p + 4 < end) lo |= (uint64_t)load_dword(bytes, nbytes, p + 4) << 32;
  uint64_t w = lo >> sh;
  if (sh && p + 8 < end) w |= (uint64_t)load_dword(bytes, nbytes, p + 8) << (64 - sh);
  w = __builtin_bswap64(w);
  uint64_t mask = avail >= 8 ? ~0ull : ~(~0ull >> (8 * avail));
  return w & mask;
}

__device__ __forceinline__ int64_t row_of(const StrView& v, uint32_t i) {
  return v.rows ? v.rows[i] : (int64_t)i;
}

__device__ __forceinline__ uint64_t build_key(const StrView& v, uint32_t i) {
  int64_t r = row_of(v, i);
  int64_t o = v.offsets[r];
  int64_t len = v.offsets[r + 1] - o;
  if (len <= 0) return 0;
  return load_be64(v.bytes, v.nbytes, o, (int)(len < 8 ? len : 8));
}

// order of two pairs whose keys are equal
__device__ __forceinline__ bool tie_less(const StrView& v, uint32_t ia, uint32_t ib) {
  if (ib >= v.m) return ia < v.m;  // padding sorts last
  if (ia >= v.m) return false;
  int64_t ra = row_of(v, ia), rb = row_of(v, ib);
  int64_t oa = v.offsets[ra], ob = v.offsets[rb];
  int64_t la = v.offsets[ra + 1] - oa, lb = v.offsets[rb + 1] - ob;
  int64_t common = la < lb ? la : lb;
  for (int64_t j = 8; j < common; j += 8) {
    int avail = (int)(common - j < 8 ? common - j : 8);
    uint64_t wa = load_be64(v.bytes, v.nbytes, oa + j, avail);
    uint64_t wb = load_be64(v.bytes, v.nbytes, ob + j, avail);
    if (wa != wb) return wa < wb;
  }
  if (la != lb) return la < lb;
  return ia < ib;
}

__device__ __forceinline__ bool pair_less(const StrView& v, uint64_t ka, uint32_t ia,
                                          uint64_t kb, uint32_t ib) {
  if (ka != kb) return ka < kb;
  return tie_less(v, ia, ib);
}

// number of A elements among the first `diag` outputs of merge(A, B)
template <typename I>
__device__ __forceinline__ I merge_path(const StrView& v, const uint64_t* ak,
                                        const uint32_t* ai, I na, const uint64_t* bk,
                                        const uint32_t* bi, I nb, I diag) {
  I lo = diag > nb ? diag - nb : 0;
  I hi = diag < na ? diag : na;
  while (lo < hi) {
    I mid = (lo + hi) >> 1;
    I b = diag - 1 - mid;
    if (pair_less(v, bk[b], bi[b], ak[mid], ai[mid])) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// kPer outputs of merge(sk[a, aend), sk[b, bend)) into registers; outputs past
// the end of both runs are unspecified
__device__ __forceinline__ void serial_merge(const StrView& v, const uint64_t* sk,
                                             const uint32_t* si, int a, int aend, int b,
                                             int bend, uint64_t (&rk)[kPer],
                                             uint32_t (&ri)[kPer]) {
  uint64_t ka = 0, kb = 0;
  uint32_t ia = 0, ib = 0;
  if (a < aend) { ka = sk[a]; ia = si[a]; }
  if (b < bend) { kb = sk[b]; ib = si[b]; }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    bool take_a = b >= bend || (a < aend && !pair_less(v, kb, ib, ka, ia));
    rk[k] = take_a ? ka : kb;
    ri[k] = take_a ? ia : ib;
    if (take_a) {
      ++a;
      if (a < aend) { ka = sk[a]; ia = si[a]; }
    } else {
      ++b;
      if (b < bend) { kb = sk[b]; ib = si[b]; }
    }
  }
}

#define SAIL_CSWAP(i, j)                                     \
  if (pair_less(v, rk[j], ri[j], rk[i], ri[i])) {            \
    uint64_t tk = rk[i]; rk[i] = rk[j]; rk[j] = tk;          \
    uint32_t ti = ri[i]; ri[i] = ri[j]; ri[j] = ti;          \
  }

__global__ __launch_bounds__(kBlock) void str_tile_sort_kernel(
    StrView v, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  __shared__ uint64_t sk[kTile];
  __shared__ uint32_t si[kTile];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  // key pass: one thread per row, rows of a wave adjacent
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    int j = t + k * kBlock;
    int64_t g = base + j;
    bool real = g < (int64_t)v.m;
    sk[j] = real ? build_key(v, (uint32_t)g) : ~0ull;
    si[j] = real ? (uint32_t)g : kPadIndex;
  }
  __syncthreads();
  uint64_t rk[kPer];
  uint32_t ri[kPer];
  const int pos = t * kPer;
#pragma unroll
  for (int k = 0; k < kPer; ++k) { rk[k] = sk[pos + k]; ri[k] = si[pos + k]; }
  SAIL_CSWAP(0, 1) SAIL_CSWAP(2, 3) SAIL_CSWAP(4, 5) SAIL_CSWAP(6, 7)
  SAIL_CSWAP(0, 2) SAIL_CSWAP(1, 3) SAIL_CSWAP(4, 6) SAIL_CSWAP(5, 7)
  SAIL_CSWAP(1, 2) SAIL_CSWAP(5, 6)
  SAIL_CSWAP(0, 4) SAIL_CSWAP(1, 5) SAIL_CSWAP(2, 6) SAIL_CSWAP(3, 7)
  SAIL_CSWAP(2, 4) SAIL_CSWAP(3, 5)
  SAIL_CSWAP(1, 2) SAIL_CSWAP(3, 4) SAIL_CSWAP(5, 6)
#pragma unroll
  for (int k = 0; k < kPer; ++k) { sk[pos + k] = rk[k]; si[pos + k] = ri[k]; }
  __syncthreads();
  for (int L = kPer; L < kTile; L <<= 1) {
    int g0 = pos & ~(2 * L - 1);
    int diag = pos - g0;
    int a = merge_path<int>(v, sk + g0, si + g0, L, sk + g0 + L, si + g0 + L, L, diag);
    serial_merge(v, sk, si, g0 + a, g0 + L, g0 + L + diag - a, g0 + 2 * L, rk, ri);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) { sk[pos + k] = rk[k]; si[pos + k] = ri[k]; }
    __syncthreads();
  }
  // padding sorted to the tile's end: the first (m - base) pairs are the rows
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    int j = t + k * kBlock;
    int64_t g = base + j;
    if (g < (int64_t)v.m) { keys[g] = sk[j]; idx[g] = si[j]; }
  }
}

// the pair of runs of length R that output tile `tile` belongs to
struct RunPair {
  int64_t a_lo, a_hi, b_hi;  // A = [a_lo, a_hi), B = [a_hi, b_hi)
  int64_t d0;                // the tile's first output, counted within the pair
};

__device__ __forceinline__ RunPair run_pair(int64_t tile, int64_t R, int64_t m) {
  RunPair p;
  int64_t out0 = tile * kTile;
  p.a_lo = out0 / (2 * R) * (2 * R);
  p.a_hi = p.a_lo + R < m ? p.a_lo + R : m;
  p.b_hi = p.a_lo + 2 * R < m ? p.a_lo + 2 * R : m;
  p.d0 = out0 - p.a_lo;
  return p;
}

__global__ __launch_bounds__(kBlock) void str_merge_partition_kernel(
    StrView v, const uint64_t* __restrict__ kin, const uint32_t* __restrict__ iin,
    int64_t* __restrict__ mp, int64_t R, int64_t ntiles) {
  int64_t tile = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (tile >= ntiles) return;
  RunPair p = run_pair(tile, R, (int64_t)v.m);
  mp[tile] = merge_path<int64_t>(v, kin + p.a_lo, iin + p.a_lo, p.a_hi - p.a_lo,
                                 kin + p.a_hi, iin + p.a_hi, p.b_hi - p.a_hi, p.d0);
}

__global__ __launch_bounds__(kBlock) void str_merge_kernel(
    StrView v, const uint64_t* __restrict__ kin, const uint32_t* __restrict__ iin,
    uint64_t* __restrict__ kout, uint32_t* __restrict__ iout,
    const int64_t* __restrict__ mp, int64_t R) {
  __shared__ uint64_t sk[kTile];
  __shared__ uint32_t si[kTile];
  const int t = threadIdx.x;
  const int64_t tile = blockIdx.x;
  RunPair p = run_pair(tile, R, (int64_t)v.m);
  int64_t len_a = p.a_hi - p.a_lo, len_b = p.b_hi - p.a_hi;
  int64_t d1 = p.d0 + kTile < len_a + len_b ? p.d0 + kTile : len_a + len_b;
  // a diagonal short of the pair's end is the next tile's, in the same pair
  int64_t a0 = mp[tile];
  int64_t a1 = d1 == len_a + len_b ? len_a : mp[tile + 1];
  int64_t b0 = p.d0 - a0;
  int na = (int)(a1 - a0), n = (int)(d1 - p.d0);  // n <= kTile
  for (int j = t; j < n; j += kBlock) {
    int64_t src = j < na ? p.a_lo + a0 + j : p.a_hi + b0 + (j - na);
    sk[j] = kin[src];
    si[j] = iin[src];
  }
  __syncthreads();
  uint64_t rk[kPer];
  uint32_t ri[kPer];
  const int pos = t * kPer;
  int diag = pos < n ? pos : n;
  int a = merge_path<int>(v, sk, si, na, sk + na, si + na, n - na, diag);
  serial_merge(v, sk, si, a, na, na + diag - a, n, rk, ri);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPer; ++k) { sk[pos + k] = rk[k]; si[pos + k] = ri[k]; }
  __syncthreads();
  const int64_t out0 = tile * kTile;
  for (int j = t; j < n; j += kBlock) {
    kout[out0 + j] = sk[j];
    iout[out0 + j] = si[j];
  }
}

__global__ void str_emit_rows_kernel(const uint32_t* __restrict__ idx,
                                     const int64_t* __restrict__ rows,
                                     int64_t* __restrict__ out, int64_t m) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += gridDim.x * (int64_t)blockDim.x) {
    uint32_t j = idx[i];
    out[i] = rows ? rows[j] : (int64_t)j;
  }
}

// three-way compare of bytes_a[oa, oa+la) and bytes_b[ob, ob+lb)
__device__ __forceinline__ int compare3(const uint8_t* bytes_a, int64_t nbytes_a,
                                        int64_t oa, int64_t la, const uint8_t* bytes_b,
                                        int64_t nbytes_b, int64_t ob, int64_t lb) {
  int64_t common = la < lb ? la : lb;
  for (int64_t j = 0; j < common; j += 8) {
    int avail = (int)(common - j < 8 ? common - j : 8);
    uint64_t wa = load_be64(bytes_a, nbytes_a, oa + j, avail);
    uint64_t wb = load_be64(bytes_b, nbytes_b, ob + j, avail);
    if (wa != wb) return wa < wb ? -1 : 1;
  }
  return la == lb ? 0 : (la < lb ? -1 : 1);
}

__global__ void str_rank_flags_kernel(const int64_t* __restrict__ offsets,
                                      const uint8_t* __restrict__ bytes, int64_t nbytes,
                                      const int64_t* __restrict__ perm,
                                      uint8_t* __restrict__ flag, int64_t m) {
  // flag[i] = 1 where sorted position i starts a new value
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m;
       i += gridDim.x * (int64_t)blockDim.x) {
    if (i == 0) { flag[0] = 0; continue; }
    int64_t ra = perm[i - 1], rb = perm[i];
    int64_t oa = offsets[ra], ob = offsets[rb];
    int64_t la = offsets[ra + 1] - oa, lb = offsets[rb + 1] - ob;
    flag[i] = la != lb ||
              compare3(bytes, nbytes, oa, la, bytes, nbytes, ob, lb) != 0;
  }
}

__global__ void str_compare3_kernel(const int64_t* __restrict__ offs_a,
                                    const uint8_t* __restrict__ bytes_a, int64_t nbytes_a,
                                    const int64_t* __restrict__ offs_b,
                                    const uint8_t* __restrict__ bytes_b, int64_t nbytes_b,
                                    int64_t b_stride, int8_t* __restrict__ out,
                                    int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * (int64_t)blockDim.x) {
    int64_t ib = i * b_stride;  // stride 0: one broadcast value
    int64_t oa = offs_a[i], ob = offs_b[ib];
    out[i] = (int8_t)compare3(bytes_a, nbytes_a, oa, offs_a[i + 1] - oa, bytes_b,
                              nbytes_b, ob, offs_b[ib + 1] - ob);
  }
}

void check_strings(const torch::Tensor& offsets, const torch::Tensor& bytes) {
  SAIL_CHECK(offsets.is_cuda() && bytes.is_cuda());
  SAIL_CHECK(offsets.device() == bytes.device());
  SAIL_CHECK(offsets.scalar_type() == torch::kInt64);
  SAIL_CHECK(bytes.scalar_type() == torch::kUInt8);
  SAIL_CHECK(offsets.is_contiguous() && bytes.is_contiguous());
  SAIL_CHECK(offsets.dim() == 1 && bytes.dim() == 1);
  SAIL_CHECK(offsets.numel() >= 1);
}

void check_index(const torch::Tensor& idx, const torch::Tensor& offsets) {
  SAIL_CHECK(idx.is_cuda() && idx.device() == offsets.device());
  SAIL_CHECK(idx.scalar_type() == torch::kInt64);
  SAIL_CHECK(idx.is_contiguous() && idx.dim() == 1);
}

// the word loads want a 4-byte aligned base; a view that is not gets a copy
torch::Tensor aligned_bytes(const torch::Tensor& bytes) {
  if (reinterpret_cast<uintptr_t>(bytes.data_ptr()) % 4 == 0) return bytes;
  return bytes.clone();
}

}  // namespace

torch::Tensor str_sort_perm(torch::Tensor offsets, torch::Tensor bytes,
                            c10::optional<torch::Tensor> rows) {
  check_strings(offsets, bytes);
  SAIL_DEVICE_GUARD(offsets);
  int64_t n = offsets.numel() - 1;
  int64_t m = n;
  const int64_t* rows_p = nullptr;
  if (rows.has_value()) {
    check_index(*rows, offsets);
    m = rows->numel();
    rows_p = rows->data_ptr<int64_t>();
    SAIL_CHECK(m == 0 || n > 0);
  }
  TORCH_CHECK(m < (int64_t(1) << 32), "str_sort_perm: ", m, " rows, limit 2^32 - 1");
  auto i64 = offsets.options().dtype(torch::kInt64);
  if (m == 0) return torch::empty({0}, i64);
  if (m == 1) return rows.has_value() ? rows->clone() : torch::zeros({1}, i64);

  bytes = aligned_bytes(bytes);
  int64_t ntiles = (m + kTile - 1) / kTile;
  auto out = torch::empty({m}, i64);
  auto key_buf = torch::empty({ntiles > 1 ? 2 : 1, m}, i64);
  auto idx_buf = torch::empty({ntiles > 1 ? 2 : 1, m}, offsets.options().dtype(torch::kInt32));
  auto mp = torch::empty({ntiles}, i64);

  StrView v{offsets.data_ptr<int64_t>(), bytes.data_ptr<uint8_t>(), bytes.numel(), rows_p,
            (uint32_t)m};
  uint64_t* kb[2];
  uint32_t* ib[2];
  for (int s = 0; s < 2; ++s) {
    int64_t at = ntiles > 1 ? s * m : 0;
    kb[s] = reinterpret_cast<uint64_t*>(key_buf.data_ptr<int64_t>()) + at;
    ib[s] = reinterpret_cast<uint32_t*>(idx_buf.data_ptr<int32_t>()) + at;
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(str_tile_sort_kernel, dim3((unsigned)ntiles), dim3(kBlock), 0, stream,
                     v, kb[0], ib[0]);
  int cur = 0;
  for (int64_t R = kTile; R < m; R *= 2) {
    hipLaunchKernelGGL(str_merge_partition_kernel,
                       dim3((unsigned)((ntiles + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       stream, v, kb[cur], ib[cur], mp.data_ptr<int64_t>(), R, ntiles);
    hipLaunchKernelGGL(str_merge_kernel, dim3((unsigned)ntiles), dim3(kBlock), 0, stream, v,
                       kb[cur], ib[cur], kb[cur ^ 1], ib[cur ^ 1], mp.data_ptr<int64_t>(),
                       R);
    cur ^= 1;
  }
  hipLaunchKernelGGL(str_emit_rows_kernel, dim3(grid_for(m)), dim3(kBlock), 0, stream,
                     ib[cur], rows_p, out.data_ptr<int64_t>(), m);
  return out;
}

std::vector<torch::Tensor> str_dense_rank(torch::Tensor offsets, torch::Tensor bytes,
                                          torch::Tensor perm) {
  check_strings(offsets, bytes);
  check_index(perm, offsets);
  SAIL_DEVICE_GUARD(offsets);
  int64_t m = perm.numel();
  auto i64 = offsets.options().dtype(torch::kInt64);
  if (m == 0) return {torch::empty({0}, i64), torch::zeros({1}, i64)};
  SAIL_CHECK(offsets.numel() >= 2);
  bytes = aligned_bytes(bytes);
  auto flag = torch::empty({m}, bytes.options());
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(str_rank_flags_kernel, dim3(grid_for(m)), dim3(kBlock), 0, stream,
                     offsets.data_ptr<int64_t>(), bytes.data_ptr<uint8_t>(), bytes.numel(),
                     perm.data_ptr<int64_t>(), flag.data_ptr<uint8_t>(), m);
  auto rank_sorted = flag.cumsum(0, torch::kInt64);
  return {rank_sorted, rank_sorted.slice(0, m - 1, m) + 1};
}

torch::Tensor str_compare3(torch::Tensor offs_a, torch::Tensor bytes_a,
                           torch::Tensor offs_b, torch::Tensor bytes_b) {
  check_strings(offs_a, bytes_a);
  check_strings(offs_b, bytes_b);
  SAIL_CHECK(offs_a.device() == offs_b.device());
  SAIL_DEVICE_GUARD(offs_a);
  int64_t n = offs_a.numel() - 1, nb = offs_b.numel() - 1;
  TORCH_CHECK(nb == n || nb == 1, "str_compare3: b has ", nb, " rows, a has ", n);
  auto out = torch::empty({n}, offs_a.options().dtype(torch::kInt8));
  if (n == 0) return out;
  bytes_a = aligned_bytes(bytes_a);
  bytes_b = aligned_bytes(bytes_b);
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(str_compare3_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream,
                     offs_a.data_ptr<int64_t>(), bytes_a.data_ptr<uint8_t>(),
                     bytes_a.numel(), offs_b.data_ptr<int64_t>(),
                     bytes_b.data_ptr<uint8_t>(), bytes_b.numel(),
                     (int64_t)(nb == n ? 1 : 0), out.data_ptr<int8_t>(), n);
  return out;
}
