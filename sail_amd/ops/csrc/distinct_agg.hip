// COUNT / SUM / AVG (DISTINCT x) per group for MI355X (gfx950): one pass over
// the rows and one exact hash set of (gid, key) pairs in HBM, in place of two
// 64-bit sorts, five gathers and an index_add_ per output.
//
// A pair is 128 bits and no two-word slot can be claimed by one atomic, so
// the general table stores ROW NUMBERS: a slot is uint32 `row + 1`, 0 = empty.
// A thread that meets an empty slot claims it with one 32-bit CAS; a thread
// that meets row r compares its pair with gid[r], keys[r] of the immutable
// input and is either a duplicate (done) or moves on to the next slot. What a
// claimed slot points at never changes, so a slot is complete the moment it
// is claimed: nobody ever waits for another thread. Only the thread whose CAS
// claimed a slot counts the pair, so count and sum depend on the SET of pairs
// alone: exact, and the same from run to run whichever row wins.
//
//  ONE   (gid absent, ng == 1): the table stores the 64-bit key itself, as
//        claim_slot in hash_join.hip does (slot tmask + 1 belongs to the one
//        key whose bits are the empty marker); no verify reads, no gid loads.
//        Claims are summed in registers and leave once per wave.
//  WAVE  a lane whose pair equals that of the live lane before it skips the
//        insert (sorted and clustered input).
//  CACHE a direct-mapped, claim-once LDS table of pairs this workgroup has
//        already sent to the table; a hit skips the global probe. An entry is
//        claimed by CAS of its tag to kBusy, the key is written, and the tag
//        gid + 1 is stored last with release order; readers load the tag with
//        acquire order first. A reader never takes a half-written entry for a
//        match; a miss only costs a probe.
//  LDSACC (ng <= kLdsGroups) per-workgroup LDS counters and sums, flushed
//        once; above that, global atomics. Either way adjacent claiming lanes
//        of one gid are first reduced to one update (segmented wave sum).
//
// What ships (tools/distinct_bench.py, 100M rows on one MI355X, table in
// profiles/README.md): WAVE is on, it takes input ordered by (group, value)
// with 8 copies of a pair from 4.6 ms to 1.4 ms and is within the spread
// everywhere else. CACHE is off: it lost 5 - 25 % in every case, also with
// half of the rows on 1000 hot pairs (the table's hot slots sit in L2 and the
// walk reads before it writes); it stays reachable through `variant`.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

namespace {

constexpr int kBlock = 256;             // rows per tile = threads per workgroup
constexpr int kTilesMin = 16;           // a workgroup walks >= 16 tiles
constexpr int kGridMax = 2048;
constexpr int kCacheSlots = 2048;       // 12 B each: 24 KB of LDS
constexpr int kLdsGroups = 1024;        // 16 B each: 16 KB of LDS
constexpr unsigned kBusy = 0xffffffffu; // cache tag of an entry being written
constexpr long long kEmpty = 0x8000000000000001ll;  // ONE: empty slot marker
constexpr long long kTaken = 0;                     // ONE: slot tmask + 1 in use

__device__ inline uint64_t mix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// Insert `k` into the key table of the ONE variant; true for the claimant.
__device__ inline bool claim_key(long long* __restrict__ tkeys, long long k,
                                 uint64_t h, uint64_t tmask) {
  if (k == kEmpty)
    return atomicCAS((unsigned long long*)&tkeys[tmask + 1], (unsigned long long)kEmpty,
                     (unsigned long long)kTaken) == (unsigned long long)kEmpty;
  while (true) {
    long long cur = tkeys[h];  // a stale read shows kEmpty at worst: the CAS decides
    if (cur == kEmpty)
      cur = (long long)atomicCAS((unsigned long long*)&tkeys[h], (unsigned long long)kEmpty,
                                 (unsigned long long)k);
    if (cur == kEmpty) return true;
    if (cur == k) return false;
    h = (h + 1) & tmask;
  }
}

// Insert row `row` = (g, k) into the row-number table; true for the claimant.
// The table has more slots than rows, so every walk ends at an empty slot or
// at a row holding the same pair; rows read back are below n by construction.
template <typename GidT>
__device__ inline bool claim_row(unsigned* __restrict__ trows, unsigned row, int g,
                                 long long k, const GidT* __restrict__ gid,
                                 const long long* __restrict__ keys, uint64_t h,
                                 uint64_t tmask) {
  while (true) {
    unsigned cur = trows[h];   // stale reads show 0 at worst: the CAS decides
    if (cur == 0) cur = atomicCAS(&trows[h], 0u, row + 1);
    if (cur == 0) return true;
    const unsigned r = cur - 1;  // the loser of a CAS examines the winner here
    if (keys[r] == k && (int)gid[r] == g) return false;
    h = (h + 1) & tmask;
  }
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

template <typename GidT, bool ONE, bool WAVE, bool CACHE, bool LDSACC>
__global__ __launch_bounds__(kBlock) void distinct_acc_kernel(
    const GidT* __restrict__ gid, const long long* __restrict__ keys,
    const uint8_t* __restrict__ mask, int64_t n, int64_t rows_per_block,
    void* __restrict__ table, uint64_t tmask,
    unsigned long long* __restrict__ out /* [2][ng] */, int ng, bool want_sum) {
  static_assert(!(ONE && LDSACC), "the ONE variant accumulates in registers");
  __shared__ unsigned ctag[CACHE ? kCacheSlots : 1];
  __shared__ long long ckey[CACHE ? kCacheSlots : 1];
  __shared__ unsigned long long lcnt[LDSACC ? kLdsGroups : 1];
  __shared__ unsigned long long lsum[LDSACC ? kLdsGroups : 1];
  if constexpr (CACHE)
    for (int s = threadIdx.x; s < kCacheSlots; s += kBlock) ctag[s] = 0;
  if constexpr (LDSACC)
    for (int s = threadIdx.x; s < ng; s += kBlock) lcnt[s] = lsum[s] = 0;
  if constexpr (CACHE || LDSACC) __syncthreads();

  const int lane = threadIdx.x & 63;
  unsigned long long my_cnt = 0, my_sum = 0;  // ONE: claims of this thread
  const int64_t begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t end = begin + rows_per_block < n ? begin + rows_per_block : n;
  // the loop bound is the same for the whole workgroup: every lane reaches
  // every shuffle and ballot below
  for (int64_t base = begin; base < end; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    bool live = i < end && (!mask || mask[i]);
    long long k = 0;
    int g = 0;
    if (live) {
      k = keys[i];
      if constexpr (!ONE) {
        const GidT raw = gid[i];
        live = raw >= 0 && raw < (GidT)ng;  // a gid outside [0, ng) is dropped
        g = live ? (int)raw : 0;
      }
    }

    bool insert = live;
    if constexpr (WAVE) {
      const long long kprev = __shfl_up(k, 1, 64);
      const int gprev = __shfl_up(g, 1, 64);
      const int lprev = __shfl_up((int)live, 1, 64);
      if (lane > 0 && lprev && kprev == k && gprev == g) insert = false;
    }

    bool claimed = false;
    if (insert) {
      uint64_t h = mix64((uint64_t)k);
      if constexpr (!ONE) h = mix64(h ^ ((uint64_t)(unsigned)g * 0x9e3779b97f4a7c15ull));
      if constexpr (CACHE) {
        const int s = (int)(h >> 40) & (kCacheSlots - 1);
        const unsigned tag = (unsigned)g + 1;
        unsigned t = __hip_atomic_load(&ctag[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (t == tag && ckey[s] == k) {
          insert = false;  // this workgroup has sent the pair to the table
        } else if (t == 0 && atomicCAS(&ctag[s], 0u, kBusy) == 0u) {
          ckey[s] = k;
          __hip_atomic_store(&ctag[s], tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      if (insert) {
        if constexpr (ONE)
          claimed = claim_key((long long*)table, k, h & tmask, tmask);
        else
          claimed = claim_row<GidT>((unsigned*)table, (unsigned)i, g, k, gid, keys,
                                    h & tmask, tmask);
      }
    }

    if constexpr (ONE) {
      my_cnt += claimed ? 1 : 0;
      my_sum += claimed ? (unsigned long long)k : 0ull;
    } else {
      const unsigned long long any = __ballot(claimed);
      if (any == 0) continue;  // the same for the whole wave
      // adjacent claiming lanes of one gid form a run; its first lane takes
      // the run's count and sum (hash_agg.hip's segmented reduction)
      const int gprev = __shfl_up(g, 1, 64);
      const int cprev = __shfl_up((int)claimed, 1, 64);
      const bool head = claimed && (lane == 0 || !cprev || gprev != g);
      const unsigned long long heads = __ballot(head);
      unsigned cnt = claimed ? 1u : 0u;
      unsigned long long sum = claimed && want_sum ? (unsigned long long)k : 0ull;
      if (heads != any) {
        const unsigned long long after = (heads >> lane) >> 1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const bool join = lane + off < 64 && (after & ((1ull << off) - 1)) == 0;
          const unsigned oc = __shfl_down(cnt, off, 64);
          if (join) cnt += oc;
          if (want_sum) {
            const unsigned long long os = __shfl_down(sum, off, 64);
            if (join) sum += os;
          }
        }
      }
      if (head) {
        if constexpr (LDSACC) {
          atomicAdd(&lcnt[g], (unsigned long long)cnt);
          if (want_sum) atomicAdd(&lsum[g], sum);
        } else {
          atomicAdd(&out[g], (unsigned long long)cnt);
          if (want_sum) atomicAdd(&out[(int64_t)ng + g], sum);
        }
      }
    }
  }

  if constexpr (ONE) {
    my_cnt = wave_sum(my_cnt);
    if (want_sum) my_sum = wave_sum(my_sum);
    if (lane == 0 && my_cnt) {
      atomicAdd(&out[0], my_cnt);
      if (want_sum) atomicAdd(&out[1], my_sum);
    }
  }
  if constexpr (LDSACC) {
    __syncthreads();
    for (int s = threadIdx.x; s < ng; s += kBlock) {
      if (lcnt[s] == 0) continue;
      atomicAdd(&out[s], lcnt[s]);
      if (want_sum) atomicAdd(&out[(int64_t)ng + s], lsum[s]);
    }
  }
}

struct Launch {
  int grid;
  hipStream_t stream;
  const void* gid;
  const long long* keys;
  const uint8_t* mask;
  int64_t n, rows_per_block;
  void* table;
  uint64_t tmask;
  unsigned long long* out;
  int ng;
  bool want_sum;
};

template <typename GidT, bool ONE, bool WAVE, bool CACHE, bool LDSACC>
void launch(const Launch& a) {
  hipLaunchKernelGGL((distinct_acc_kernel<GidT, ONE, WAVE, CACHE, LDSACC>), dim3(a.grid),
                     dim3(kBlock), 0, a.stream, (const GidT*)a.gid, a.keys, a.mask, a.n,
                     a.rows_per_block, a.table, a.tmask, a.out, a.ng, a.want_sum);
}

template <typename GidT, bool ONE, bool LDSACC>
void launch_flags(const Launch& a, bool wave, bool cache) {
  if (wave && cache) launch<GidT, ONE, true, true, LDSACC>(a);
  else if (wave) launch<GidT, ONE, true, false, LDSACC>(a);
  else if (cache) launch<GidT, ONE, false, true, LDSACC>(a);
  else launch<GidT, ONE, false, false, LDSACC>(a);
}

template <typename GidT>
void launch_general(const Launch& a, bool wave, bool cache) {
  if (a.ng <= kLdsGroups) launch_flags<GidT, false, true>(a, wave, cache);
  else launch_flags<GidT, false, false>(a, wave, cache);
}

}  // namespace

// int64 [2, ng]: row 0 the number of distinct (gid, key) pairs per group among
// the rows the mask keeps, row 1 the sum of those distinct keys modulo 2^64
// (zeros unless want_sum). gid absent: ng == 1 and the key-table variant; an
// explicit gid takes the row-number table whatever ng is. table_slots
// overrides the table size (a power of two above n); variant bit 0 switches
// the wave filter off and bit 1 the LDS cache on (tools/distinct_bench.py).
// Launches on the tensors' device and the current stream; never synchronises.
torch::Tensor distinct_acc(c10::optional<torch::Tensor> gid, torch::Tensor keys,
                           c10::optional<torch::Tensor> mask, int64_t ng, bool want_sum,
                           int64_t table_slots, int64_t variant) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous() && keys.scalar_type() == torch::kInt64,
              "distinct_acc: keys must be a contiguous cuda int64 tensor");
  const int64_t n = keys.numel();
  TORCH_CHECK(ng >= 1 && ng < (int64_t(1) << 31), "distinct_acc: ng must be in [1, 2^31)");
  TORCH_CHECK(n < (int64_t(1) << 32) - 1, "distinct_acc: at most 2^32 - 2 rows");
  TORCH_CHECK(variant >= 0 && variant <= 3, "distinct_acc: variant is 0..3");
  const bool one = !(gid.has_value() && gid->defined());
  TORCH_CHECK(!one || ng == 1, "distinct_acc: ng > 1 needs group ids");
  if (!one)
    TORCH_CHECK(gid->is_cuda() && gid->is_contiguous() && gid->numel() == n &&
                    gid->device() == keys.device() &&
                    (gid->scalar_type() == torch::kInt32 || gid->scalar_type() == torch::kInt64),
                "distinct_acc: gid must be a contiguous cuda int32 or int64 tensor of keys' "
                "length on keys' device");
  const uint8_t* mptr = nullptr;
  if (mask.has_value() && mask->defined()) {
    TORCH_CHECK(mask->scalar_type() == torch::kBool || mask->scalar_type() == torch::kUInt8,
                "distinct_acc: mask must be bool or uint8");
    TORCH_CHECK(mask->is_cuda() && mask->is_contiguous() && mask->numel() == n &&
                    mask->device() == keys.device(),
                "distinct_acc: mask must be a contiguous cuda tensor of keys' length on "
                "keys' device");
    mptr = (const uint8_t*)mask->data_ptr();
  }
  // more slots than rows: every probe walk ends at an empty slot
  int64_t slots = table_slots;
  if (slots == 0) {
    slots = 64;
    while (slots < 2 * n) slots <<= 1;
  }
  TORCH_CHECK(slots > n && (slots & (slots - 1)) == 0,
              "distinct_acc: table_slots must be a power of two greater than the row count");

  c10::DeviceGuard guard(keys.device());
  auto out = torch::zeros({2, ng}, keys.options());
  if (n == 0) return out;
  // allocated and filled before the launch; the ONE table has one slot more
  auto table = one ? torch::full({slots + 1}, kEmpty, keys.options())
                   : torch::zeros({slots}, keys.options().dtype(torch::kInt32));
  const int64_t tiles = (n + kBlock - 1) / kBlock;
  const int64_t grid = std::min<int64_t>((tiles + kTilesMin - 1) / kTilesMin, kGridMax);
  Launch a;
  a.grid = (int)grid;
  a.stream = c10::hip::getCurrentHIPStream();
  a.gid = one ? nullptr : gid->data_ptr();
  a.keys = (const long long*)keys.data_ptr<int64_t>();
  a.mask = mptr;
  a.n = n;
  a.rows_per_block = (tiles + grid - 1) / grid * kBlock;
  a.table = table.data_ptr();
  a.tmask = (uint64_t)slots - 1;
  a.out = (unsigned long long*)out.data_ptr<int64_t>();
  a.ng = (int)ng;
  a.want_sum = want_sum;
  // shipped: wave filter on, LDS cache off (see the header comment)
  const bool wave = !(variant & 1), cache = (variant & 2) != 0;
  if (one) launch_flags<int32_t, true, false>(a, wave, cache);
  else if (gid->scalar_type() == torch::kInt64) launch_general<int64_t>(a, wave, cache);
  else launch_general<int32_t>(a, wave, cache);
  hipError_t e = hipGetLastError();
  TORCH_CHECK(e == hipSuccess, "distinct_acc launch failed: ", hipGetErrorString(e));
  return out;
}
