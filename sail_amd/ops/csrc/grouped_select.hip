// Exact k-th value per group (median, percentile, percentile_disc) for MI355X
// (gfx950) by radix select: no sort, no gather, no compaction, no host loop.
//
// A key is the double's 64 bits made order-preserving (negatives: all bits
// flipped, otherwise the sign bit flipped), so unsigned key order is numeric
// order with -0.0 below +0.0; every NaN takes the all-ones key and sorts last.
// Eight passes of eight bits, most significant first, settle one byte of each
// group's answer per pass. The state per group lives in global memory: the key
// prefix settled so far and the rank still wanted among the rows that share it.
//
//  HIST  (one launch per pass) a workgroup walks a contiguous chunk of rows,
//        lane i on row base + i; gid, vals and mask are read once, coalesced.
//        A row takes part when the mask keeps it and its key agrees with its
//        group's prefix, and adds 1 to bin `digit` of its group: in an LDS
//        [ng][256] table flushed once for ng <= kLdsGroups, by global atomics
//        above. Before any atomic the wave combines: the lanes whose
//        (gid, digit) equals the first unserved lane's leave through one add
//        of their popcount, for kRounds rounds; what is left adds for itself.
//        The top bytes of a double are sign and exponent, so in passes 0 and 1
//        a real column fills one or two bins and the rounds take nearly all.
//  PICK  (one wave per group, after each HIST) four bins per lane, a wave scan,
//        the bin that holds the rank; its digit joins the prefix, the counts
//        below it leave the rank, the bins are cleared for the next pass. Pass
//        0 also stores the group's row count and derives the rank from q.
//        After pass 7 the bin's count is the number of rows equal to the
//        answer and the rank is the position inside that run.
//  NEIGHBOUR (one more walk) the smallest key above the answer (what a
//        continuous percentile interpolates towards), the smallest row that
//        holds the answer, and whether the group has a NaN. Both minima are
//        64-bit atomic mins, in LDS for ng <= kLdsGroups; a lane that cannot
//        lower the stored value skips, the rest are reduced per wave first.
//  FINISH decodes lo, and hi = lo when the rank's successor lies inside the
//        run of equal keys, else the neighbour (lo again when there is none).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

namespace {

constexpr int kBlock = 256;        // rows per tile = threads per workgroup
constexpr int kTilesMin = 16;      // a workgroup walks >= 16 tiles
constexpr int kGridMax = 2048;
constexpr int kBins = 256;         // one byte per pass
constexpr int kLdsGroups = 32;     // [32][256] uint32 = 32 KB of LDS
constexpr int kCacheSlots = 4096;  // 8 B each: 32 KB of LDS above kLdsGroups
constexpr int kRounds = 4;         // wave combining rounds before own atomics
constexpr int64_t kMaxGroups = int64_t(1) << 18;  // 256 MiB of bins
constexpr unsigned long long kNone = ~0ull;
constexpr unsigned long long kSign = 1ull << 63;

using u64 = unsigned long long;

__device__ inline u64 to_key(double v) {
  if (v != v) return kNone;
  const u64 b = (u64)__double_as_longlong(v);
  return (b & kSign) ? ~b : (b | kSign);
}

__device__ inline double from_key(u64 k) {
  return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k));
}

// Row i of the walk: its key and group, and whether it counts at all.
template <typename GidT, bool ONE>
__device__ inline bool load_row(const GidT* __restrict__ gid, const double* __restrict__ vals,
                                const uint8_t* __restrict__ mask, int64_t i, int64_t end,
                                int ng, u64& key, int& g) {
  key = 0;
  g = 0;
  bool live = i < end && (!mask || mask[i]);
  if (live) {
    key = to_key(vals[i]);
    if constexpr (!ONE) {
      const GidT raw = gid[i];
      live = raw >= 0 && raw < (GidT)ng;  // a gid outside [0, ng) is dropped
      g = live ? (int)raw : 0;
    }
  }
  return live;
}

template <typename GidT, bool ONE, bool LDSH, bool FIRST>
__global__ __launch_bounds__(kBlock) void select_hist_kernel(
    const GidT* __restrict__ gid, const double* __restrict__ vals,
    const uint8_t* __restrict__ mask, int64_t n, int64_t rows_per_block,
    const u64* __restrict__ prefix, unsigned* __restrict__ hist, int ng, int shift) {
  __shared__ unsigned lh[LDSH ? kLdsGroups * kBins : 1];
  __shared__ unsigned ctag[LDSH ? 1 : kCacheSlots];
  __shared__ unsigned ccnt[LDSH ? 1 : kCacheSlots];
  if constexpr (LDSH) {
    for (int s = threadIdx.x; s < ng * kBins; s += kBlock) lh[s] = 0;
  } else {
    for (int s = threadIdx.x; s < kCacheSlots; s += kBlock) ctag[s] = ccnt[s] = 0;
  }
  __syncthreads();
  // c rows into `bin`: the LDS table; above kLdsGroups the bin's cache slot
  // when this workgroup's first comer to the slot was this bin, else HBM
  auto add = [&](u64 bin, unsigned c) {
    if constexpr (LDSH) {
      atomicAdd(&lh[bin], c);
    } else {
      const unsigned tag = (unsigned)bin + 1;            // bin < 2^26
      const unsigned s = (tag * 2654435761u) >> 20;      // 12 bits: < kCacheSlots
      unsigned t = __hip_atomic_load(&ctag[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (t == 0) {
        t = atomicCAS(&ctag[s], 0u, tag);                // a tag never changes once set
        if (t == 0) t = tag;
      }
      if (t == tag) atomicAdd(&ccnt[s], c);
      else atomicAdd(&hist[bin], c);
    }
  };
  const int lane = threadIdx.x & 63;
  const int64_t begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t end = begin + rows_per_block < n ? begin + rows_per_block : n;
  // the loop bound is the same for the whole workgroup: every lane reaches
  // every shuffle and ballot below
  for (int64_t base = begin; base < end; base += kBlock) {
    u64 key;
    int g;
    bool pending = load_row<GidT, ONE>(gid, vals, mask, base + threadIdx.x, end, ng, key, g);
    if constexpr (!FIRST) {
      // shift + 8 <= 56: the bytes above this pass's digit
      if (pending) pending = ((key ^ prefix[g]) >> (shift + 8)) == 0;
    }
    const u64 bin = ((u64)(unsigned)g << 8) | ((key >> shift) & 255u);  // < ng * 256
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const u64 act = __ballot(pending);
      if (act == 0) break;  // the same for the whole wave
      const int leader = __ffsll((long long)act) - 1;
      const u64 lbin = __shfl(bin, leader, 64);
      const bool match = pending && bin == lbin;
      const u64 m = __ballot(match);
      if (lane == leader) add(bin, (unsigned)__popcll(m));
      pending = pending && !match;
    }
    if (pending) add(bin, 1u);
  }
  __syncthreads();
  if constexpr (LDSH) {
    for (int s = threadIdx.x; s < ng * kBins; s += kBlock)
      if (lh[s]) atomicAdd(&hist[s], lh[s]);
  } else {
    for (int s = threadIdx.x; s < kCacheSlots; s += kBlock)
      if (ccnt[s]) atomicAdd(&hist[ctag[s] - 1], ccnt[s]);
  }
}

// The wanted 0-based rank among n_g sorted rows, in double arithmetic as the
// host code has it: numpy's floor((n - 1) * q) for the continuous mode, the
// smallest value with cdf >= q for the discrete ones.
__device__ inline u64 wanted_rank(u64 n_g, double q, double qq, int mode) {
  const double last = (double)(n_g - 1);
  double r;
  if (mode == 0) {
    r = floor(qq * last);
  } else {
    r = ceil(q * (double)n_g) - 1.0;
    r = r < 0.0 ? 0.0 : r;
  }
  r = r > last ? last : r;
  r = r < 0.0 ? 0.0 : r;
  return mode == 2 ? n_g - 1 - (u64)r : (u64)r;
}

template <bool FIRST>
__global__ __launch_bounds__(kBlock) void select_pick_kernel(
    unsigned* __restrict__ hist, u64* __restrict__ prefix, u64* __restrict__ rank,
    u64* __restrict__ run, int64_t* __restrict__ count, int ng, int shift, double q, double qq,
    int mode) {
  const int g = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (g >= ng) return;  // a whole wave leaves
  const int lane = threadIdx.x & 63;
  uint4* bins = (uint4*)(hist + (int64_t)g * kBins);
  const uint4 b = bins[lane];
  bins[lane] = make_uint4(0, 0, 0, 0);
  const u64 mine = (u64)b.x + b.y + b.z + b.w;
  u64 incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  const u64 total = __shfl(incl, 63, 64);
  u64 r;
  if constexpr (FIRST) {
    if (lane == 0) count[g] = (int64_t)total;
    if (total == 0) return;  // an empty group keeps prefix 0 and run 0
    r = wanted_rank(total, q, qq, mode);
  } else {
    if (total == 0) return;
    r = rank[g];
  }
  const u64 holds = __ballot(incl > r);
  if (holds == 0) return;  // cannot happen while r < total
  const int src = __ffsll((long long)holds) - 1;
  u64 below = __shfl(incl - mine, src, 64);
  const unsigned c0 = __shfl(b.x, src, 64), c1 = __shfl(b.y, src, 64),
                 c2 = __shfl(b.z, src, 64), c3 = __shfl(b.w, src, 64);
  // the first of the lane's four bins whose running count passes the rank
  int j = 0;
  unsigned c = c0;
  if (below + c0 <= r) {
    below += c0, j = 1, c = c1;
    if (below + c1 <= r) {
      below += c1, j = 2, c = c2;
      if (below + c2 <= r) below += c2, j = 3, c = c3;
    }
  }
  if (lane == 0) {
    const u64 digit = (u64)(src * 4 + j);
    prefix[g] = (FIRST ? 0ull : prefix[g]) | (digit << shift);
    rank[g] = r - below;
    run[g] = c;
  }
}

// Per-wave rounds in front of an atomic min: the lanes of the first unserved
// lane's group hand their smallest value to that lane, which issues one atomic.
template <bool ONE>
__device__ inline void wave_min_into(u64* __restrict__ dst, bool cand, int g, u64 v, int lane) {
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const u64 act = __ballot(cand);
    if (act == 0) return;  // the same for the whole wave
    const int leader = __ffsll((long long)act) - 1;
    const int lg = ONE ? 0 : __shfl(g, leader, 64);
    const bool match = cand && g == lg;
    u64 m = match ? v : kNone;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const u64 o = __shfl_xor(m, d, 64);
      m = o < m ? o : m;
    }
    if (lane == leader) atomicMin(&dst[g], m);
    cand = cand && !match;
  }
  if (cand) atomicMin(&dst[g], v);
}

template <typename GidT, bool ONE, bool LDSV>
__global__ __launch_bounds__(kBlock) void select_neighbour_kernel(
    const GidT* __restrict__ gid, const double* __restrict__ vals,
    const uint8_t* __restrict__ mask, int64_t n, int64_t rows_per_block,
    const u64* __restrict__ prefix, u64* __restrict__ next_key, u64* __restrict__ first_row,
    int64_t* __restrict__ nan_flag, int ng) {
  __shared__ u64 lnext[LDSV ? kLdsGroups : 1];
  __shared__ u64 lrow[LDSV ? kLdsGroups : 1];
  u64* nk = next_key;
  u64* fr = first_row;
  if constexpr (LDSV) {
    if (threadIdx.x < ng) lnext[threadIdx.x] = lrow[threadIdx.x] = kNone;
    __syncthreads();
    nk = lnext;
    fr = lrow;
  }
  const int lane = threadIdx.x & 63;
  const int64_t begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t end = begin + rows_per_block < n ? begin + rows_per_block : n;
  for (int64_t base = begin; base < end; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    u64 key;
    int g;
    const bool live = load_row<GidT, ONE>(gid, vals, mask, i, end, ng, key, g);
    if (live && key == kNone && nan_flag[g] == 0) nan_flag[g] = 1;  // every writer stores 1
    const u64 lo = live ? prefix[g] : 0;
    // a stale read shows a larger minimum at worst: the atomic decides
    const bool above = live && key > lo &&
                       key < __hip_atomic_load(&nk[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool equal = live && key == lo &&
                       (u64)i < __hip_atomic_load(&fr[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wave_min_into<ONE>(nk, above, g, key, lane);
    wave_min_into<ONE>(fr, equal, g, (u64)i, lane);
  }
  if constexpr (LDSV) {
    __syncthreads();
    if (threadIdx.x < ng) {
      if (lnext[threadIdx.x] != kNone) atomicMin(&next_key[threadIdx.x], lnext[threadIdx.x]);
      if (lrow[threadIdx.x] != kNone) atomicMin(&first_row[threadIdx.x], lrow[threadIdx.x]);
    }
  }
}

__global__ __launch_bounds__(kBlock) void select_finish_kernel(
    const u64* __restrict__ prefix, const u64* __restrict__ rank, const u64* __restrict__ run,
    const u64* __restrict__ next_key, const u64* __restrict__ first_row,
    const int64_t* __restrict__ count, double* __restrict__ lo_hi, int64_t* __restrict__ row,
    int ng) {
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= ng) return;
  if (count[g] == 0) {
    lo_hi[g] = lo_hi[(int64_t)ng + g] = 0.0;
    row[g] = -1;
    return;
  }
  const double lo = from_key(prefix[g]);
  const bool inside = rank[g] + 1 < run[g];
  lo_hi[g] = lo;
  lo_hi[(int64_t)ng + g] = (inside || next_key[g] == kNone) ? lo : from_key(next_key[g]);
  row[g] = (int64_t)first_row[g];
}

struct Walk {
  int grid;
  hipStream_t stream;
  const void* gid;
  const double* vals;
  const uint8_t* mask;
  int64_t n, rows_per_block;
  u64 *prefix, *next_key, *first_row;
  unsigned* hist;
  int64_t* nan_flag;
  int ng;
};

template <typename GidT, bool ONE, bool LDS>
void launch_hist(const Walk& a, int pass) {
  const int shift = 56 - 8 * pass;
  if (pass == 0)
    hipLaunchKernelGGL((select_hist_kernel<GidT, ONE, LDS, true>), dim3(a.grid), dim3(kBlock), 0,
                       a.stream, (const GidT*)a.gid, a.vals, a.mask, a.n, a.rows_per_block,
                       a.prefix, a.hist, a.ng, shift);
  else
    hipLaunchKernelGGL((select_hist_kernel<GidT, ONE, LDS, false>), dim3(a.grid), dim3(kBlock), 0,
                       a.stream, (const GidT*)a.gid, a.vals, a.mask, a.n, a.rows_per_block,
                       a.prefix, a.hist, a.ng, shift);
}

template <typename GidT, bool ONE, bool LDS>
void launch_neighbour(const Walk& a) {
  hipLaunchKernelGGL((select_neighbour_kernel<GidT, ONE, LDS>), dim3(a.grid), dim3(kBlock), 0,
                     a.stream, (const GidT*)a.gid, a.vals, a.mask, a.n, a.rows_per_block,
                     a.prefix, a.next_key, a.first_row, a.nan_flag, a.ng);
}

// pass 0..7: that histogram; pass 8: the neighbour walk
template <typename GidT, bool ONE>
void launch_walk(const Walk& a, int pass) {
  if (a.ng <= kLdsGroups) {
    if (pass < 8) launch_hist<GidT, ONE, true>(a, pass);
    else launch_neighbour<GidT, ONE, true>(a);
  } else if constexpr (!ONE) {
    if (pass < 8) launch_hist<GidT, false, false>(a, pass);
    else launch_neighbour<GidT, false, false>(a);
  }
}

}  // namespace

// (float64 [2, ng], int64 [3, ng]) per group among the rows the mask keeps:
// lo = the value at the wanted rank of the group's sorted values and hi = the
// value at the next rank (lo again at the last rank); the row count, the
// smallest row whose value is lo (-1 for a group without rows, whose lo and hi
// are 0), and 1 when the group holds a NaN. mode 0 wants rank
// floor(qq * (count - 1)) (continuous; qq is q as the caller rounded it, q
// itself when negative), mode
// 1 the smallest value whose cdf reaches q (rank ceil(q * count) - 1), mode 2
// the same counted from the largest value down. gid absent means ng == 1.
// Launches on the tensors' device and the current stream; never synchronises.
std::vector<torch::Tensor> grouped_select(torch::Tensor vals, c10::optional<torch::Tensor> gid,
                                          c10::optional<torch::Tensor> mask, int64_t ng,
                                          double q, int64_t mode, double qq) {
  TORCH_CHECK(vals.is_cuda() && vals.is_contiguous() && vals.scalar_type() == torch::kFloat64,
              "grouped_select: vals must be a contiguous cuda float64 tensor");
  const int64_t n = vals.numel();
  TORCH_CHECK(ng >= 1 && ng <= kMaxGroups, "grouped_select: ng must be in [1, 2^18]");
  TORCH_CHECK(n < (int64_t(1) << 32) - 1, "grouped_select: at most 2^32 - 2 rows");
  TORCH_CHECK(mode >= 0 && mode <= 2, "grouped_select: mode is 0, 1 or 2");
  if (qq < 0.0) qq = q;
  TORCH_CHECK(q >= 0.0 && q <= 1.0 && qq <= 1.0, "grouped_select: q must be in [0, 1]");
  const bool one = !(gid.has_value() && gid->defined());
  TORCH_CHECK(!one || ng == 1, "grouped_select: ng > 1 needs group ids");
  if (!one)
    TORCH_CHECK(gid->is_cuda() && gid->is_contiguous() && gid->numel() == n &&
                    gid->device() == vals.device() &&
                    (gid->scalar_type() == torch::kInt32 || gid->scalar_type() == torch::kInt64),
                "grouped_select: gid must be a contiguous cuda int32 or int64 tensor of vals' "
                "length on vals' device");
  const uint8_t* mptr = nullptr;
  if (mask.has_value() && mask->defined()) {
    TORCH_CHECK(mask->scalar_type() == torch::kBool || mask->scalar_type() == torch::kUInt8,
                "grouped_select: mask must be bool or uint8");
    TORCH_CHECK(mask->is_cuda() && mask->is_contiguous() && mask->numel() == n &&
                    mask->device() == vals.device(),
                "grouped_select: mask must be a contiguous cuda tensor of vals' length on "
                "vals' device");
    mptr = (const uint8_t*)mask->data_ptr();
  }

  c10::DeviceGuard guard(vals.device());
  const auto i64 = vals.options().dtype(torch::kInt64);
  // everything is allocated and filled before the first launch below
  auto lo_hi = torch::zeros({2, ng}, vals.options());
  auto meta = torch::zeros({3, ng}, i64);            // count, row, NaN flag
  if (n == 0) {
    meta.select(0, 1).fill_(-1);
    return {lo_hi, meta};
  }
  auto state = torch::zeros({3, ng}, i64);           // prefix, rank, run of equal keys
  auto mins = torch::full({2, ng}, -1, i64);         // next key, first row: kNone
  auto hist = torch::zeros({ng * kBins}, vals.options().dtype(torch::kInt32));

  const int64_t tiles = (n + kBlock - 1) / kBlock;
  const int64_t grid = std::min<int64_t>((tiles + kTilesMin - 1) / kTilesMin, kGridMax);
  u64* st = (u64*)state.data_ptr<int64_t>();
  u64* mn = (u64*)mins.data_ptr<int64_t>();
  int64_t* mt = meta.data_ptr<int64_t>();
  Walk a;
  a.grid = (int)grid;
  a.stream = c10::hip::getCurrentHIPStream();
  a.gid = one ? nullptr : gid->data_ptr();
  a.vals = vals.data_ptr<double>();
  a.mask = mptr;
  a.n = n;
  a.rows_per_block = (tiles + grid - 1) / grid * kBlock;
  a.prefix = st;
  a.next_key = mn;
  a.first_row = mn + ng;
  a.hist = (unsigned*)hist.data_ptr<int32_t>();
  a.nan_flag = mt + 2 * ng;
  a.ng = (int)ng;
  const int pick_grid = (int)((ng + kBlock / 64 - 1) / (kBlock / 64));
  for (int pass = 0; pass <= 8; ++pass) {
    if (one) launch_walk<int32_t, true>(a, pass);
    else if (gid->scalar_type() == torch::kInt64) launch_walk<int64_t, false>(a, pass);
    else launch_walk<int32_t, false>(a, pass);
    if (pass == 0)
      hipLaunchKernelGGL((select_pick_kernel<true>), dim3(pick_grid), dim3(kBlock), 0, a.stream,
                         a.hist, st, st + ng, st + 2 * ng, mt, a.ng, 56, q, qq, (int)mode);
    else if (pass < 8)
      hipLaunchKernelGGL((select_pick_kernel<false>), dim3(pick_grid), dim3(kBlock), 0, a.stream,
                         a.hist, st, st + ng, st + 2 * ng, mt, a.ng, 56 - 8 * pass, q, qq,
                         (int)mode);
  }
  hipLaunchKernelGGL(select_finish_kernel, dim3((int)((ng + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, a.stream, st, st + ng, st + 2 * ng, mn, mn + ng, mt,
                     lo_hi.data_ptr<double>(), mt + ng, a.ng);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "grouped_select launch failed: ", hipGetErrorString(e));
  return {lo_hi, meta};
}
