// PLAIN BYTE_ARRAY on the device (gfx950 / CDNA4): the length-chain index and
// the byte gather behind every plain string page and every string dictionary
// page (datasource/gpu_parquet.py).
//
// pq_bytearray_index replaces pq_bytearray_walk (parquet_decode.hip), whose
// single walking thread follows <u32 len><bytes> with four dependent byte
// loads from global memory per value. Here one wave owns a page and four
// pages share a 256-thread workgroup (no workgroup barrier anywhere: the
// waves never wait for one another, and the grid strides over the table):
//   1. the wave stages the page through LDS in windows of kWin bytes with
//      16-byte loads. Two windows form a ring; the loads of the next window
//      are issued before the current one is walked and land in LDS after it,
//      so they are in flight during the walk;
//   2. the wave follows the chain in LDS: per value one dependent LDS round
//      trip (two dword reads, the same in every lane, and a shift, so a
//      prefix may straddle the two windows of the ring). The walk's state
//      is wave-uniform and lives in scalar registers. A value longer than
//      the ring makes it skip ahead: one window load per such value, none
//      per ordinary value;
//   3. lane n keeps hop n of a batch of kBatch, and the whole wave writes
//      `lengths` and `src_pos` for the batch as two coalesced stores.
// Every length is checked against the page region before it is recorded, so
// src_pos + length never leaves [src_off, src_off + src_len). A page that
// breaks the format gets a non-zero status and length 0, src_pos = src_off
// for every row not resolved before the break:
//   1  a length runs past the end of the page
//   2  the page ends inside a length prefix, or before n_values were found
//   3  the descriptor does not fit `buf` or the outputs (nothing is written;
//      the outputs are zero-filled by the wrapper)
// A page with n_values == 0 writes nothing but its status (0).
//
// pq_gather_bytes replaces pq_gather_strings, which copies one whole value
// per thread byte by byte. Here a workgroup takes a contiguous chunk of
// values, which is a contiguous range of output bytes when out_offsets is the
// running sum of lengths (what every caller passes). It keeps the chunk's
// offsets, sources and lengths in LDS; every lane takes sixteen consecutive
// output bytes, finds the value of the first by binary search in LDS and
// steps on from there, segment by segment: a segment is the part of one
// value that lies in the lane's block. It is read as the aligned dwords
// around its source (at most five), shifted into place and merged into the
// block in registers. A lane writes its block as one 16-byte store (a wave:
// 1 KiB), and the unaligned ends of a chunk as bytes: stores are coalesced
// and a value of any length is spread over all lanes. Sources may repeat
// and overlap; lengths of 0 are legal anywhere. `buf` must be 4-byte
// aligned (the buffer contract of parquet_decode.hip).
//
// Bounds: neither kernel loads outside [buf, buf + numel) or stores outside
// its outputs for any table or any src_pos / lengths / out_offsets the host
// can hand it: descriptors are checked, 16-byte loads that would cross the
// ends of `buf` go byte by byte, a gathered byte whose source lies outside
// `buf` is written as 0, and output positions come from the loop bounds,
// never from the data. Reads past the end of a page stay inside the 16-byte
// tail of the buffer contract (parquet_decode.hip).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be a device tensor")

namespace {

typedef unsigned long long u64;

constexpr int kBlock = 256;              // 4 wave64
constexpr int kWaves = kBlock / 64;      // pages per workgroup
constexpr int kWin = 2048;               // bytes per window; the ring holds 2
constexpr int kRing = 2 * kWin;
constexpr int kPieces = kWin / 16 / 64;  // 16-byte loads per lane and window
constexpr int kBatch = 64;               // hops recorded per coalesced store

// offsets within a page are kept in 32 bits, as in parquet_delta.hip
constexpr long kPageMax = 0x7f000000L;

enum : int { kMore = 0, kNextWindow = 1, kDone = 2 };  // walk results >= 0
// walk results < 0 are minus the page status

// LDS traffic between the lanes of one wave: the wave runs one instruction
// stream and its LDS operations complete in order, so only the compiler has
// to be kept from moving accesses across this point
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ long uniform(long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(u64)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((u64)v >> 32));
  return (long)(((u64)hi << 32) | lo);
}

__global__ __launch_bounds__(kBlock) void bytearray_index_kernel(
    const uint8_t* __restrict__ buf, long buf_len,
    const long* __restrict__ pages, int npages, long* __restrict__ lengths,
    long* __restrict__ src_pos, int* __restrict__ status, long total) {
  __shared__ uint4 s_ring[kWaves][kRing / 16];

  const int lane = threadIdx.x & 63;
  // the wave's number and everything derived from it, the walk included, is
  // the same in all 64 lanes; readfirstlane tells the compiler so, and the
  // walk then runs on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint4* ring4 = s_ring[wave];
  const uint32_t* ring32 = (const uint32_t*)s_ring[wave];

  for (long p = (long)blockIdx.x * kWaves + wave; p < npages;
       p += (long)gridDim.x * kWaves) {
    const long* pgd = pages + p * 6;
    const long src_off = uniform(pgd[0]), src_len = uniform(pgd[1]);
    const long nv = uniform(pgd[2]), out_row = uniform(pgd[3]);
    if (out_row < 0 || out_row > total || nv < 0 || nv > total - out_row ||
        nv > kPageMax || src_off < 0 || src_len < 0 || src_off > buf_len ||
        src_len > buf_len - src_off) {
      if (lane == 0) status[p] = 3;
      continue;
    }
    if (nv == 0) continue;
    const int nvals = (int)nv;
    const int page_len = (int)(src_len < kPageMax ? src_len : kPageMax);
    const uint8_t* src = buf + src_off;
    // windows start on 16-byte boundaries of the address space: window k
    // holds page offsets [k * kWin - mis, (k + 1) * kWin - mis)
    const int mis = (int)((size_t)src & 15);
    long* dlen = lengths + out_row;
    long* dpos = src_pos + out_row;

    // the 16-byte pieces of window k that hold page bytes, into registers
    auto fetch = [&](int k, uint4* r) {
#pragma unroll
      for (int j = 0; j < kPieces; ++j) {
        const long c = (long)k * kWin - mis + (j * 64 + lane) * 16;  // page offset
        uint4 v = make_uint4(0, 0, 0, 0);
        if (c < page_len) {
          const long a = src_off + c;                                 // in buf
          if (a >= 0 && a + 16 <= buf_len) {
            v = *(const uint4*)(buf + a);
          } else {
            uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (a + i >= 0 && a + i < buf_len)
                q[i >> 2] |= (uint32_t)buf[a + i] << (8 * (i & 3));
            v = make_uint4(q[0], q[1], q[2], q[3]);
          }
        }
        r[j] = v;
      }
    };
    auto commit = [&](int k, const uint4* r) {
#pragma unroll
      for (int j = 0; j < kPieces; ++j)
        ring4[(k & 1) * (kWin / 16) + j * 64 + lane] = r[j];
    };

    uint4 regs[kPieces];
    int hi = 0;          // newest window in the ring
    int pos = 0;         // page offset of the next length prefix
    int found = 0;       // values resolved so far
    int st = 0;
    fetch(0, regs);
    commit(0, regs);
    while (true) {
      // the next window's loads fly while this one is walked
      fetch(hi + 1, regs);
      wave_sync();
      int res;
      while (true) {
        // prefixes that end inside window hi; they begin in hi - 1 or hi.
        // Every lane reads the same two dwords (an LDS broadcast); lane n
        // keeps hop n of the batch in its registers.
        const int win_end = (hi + 1) * kWin - mis;
        int n = 0;
        unsigned my_len = 0;
        int my_at = 0;
        res = kMore;
        while (true) {
          if (found + n >= nvals) { res = kDone; break; }
          if (n == kBatch) break;
          if (pos > page_len - 4) { res = -2; break; }
          if (pos + 4 > win_end) { res = kNextWindow; break; }
          const unsigned u = (unsigned)(pos + mis);
          const unsigned d = (u >> 2) & (kRing / 4 - 1);
          const unsigned w0 = __builtin_amdgcn_readfirstlane(ring32[d]);
          const unsigned w1 = __builtin_amdgcn_readfirstlane(
              ring32[(d + 1) & (kRing / 4 - 1)]);
          const unsigned ln =
              (unsigned)((w0 | ((u64)w1 << 32)) >> ((u & 3) * 8));
          if (ln > (unsigned)(page_len - pos - 4)) { res = -1; break; }
          if (lane == n) {
            my_len = ln;
            my_at = pos + 4;
          }
          ++n;
          pos += 4 + (int)ln;
        }
        if (lane < n) {
          dlen[found + lane] = (long)my_len;
          dpos[found + lane] = src_off + my_at;
        }
        found += n;
        if (res != kMore) break;
      }
      if (res == kDone) break;
      if (res < 0) { st = -res; break; }
      wave_sync();       // the walk's reads are done before the ring changes
      const int k = (pos + mis) / kWin;   // window of the next prefix
      if (k <= hi + 1) {
        ++hi;
        commit(hi, regs);
      } else {           // a value longer than the ring: skip ahead
        hi = k;
        fetch(hi, regs);
        commit(hi, regs);
      }
    }
    if (st != 0) {
      for (int i = found + lane; i < nvals; i += 64) {
        dlen[i] = 0;
        dpos[i] = src_off;
      }
      if (lane == 0) status[p] = st;
    }
  }
}

// ---------------------------------------------------------------------------

constexpr int kChunkMax = 512;   // values per workgroup pass

// the low n bytes of a 64-bit word set, n = 0..8
__device__ __forceinline__ u64 low_bytes(int n) {
  return n >= 8 ? ~0ull : (1ull << (8 * n)) - 1;
}

__global__ __launch_bounds__(kBlock) void gather_bytes_kernel(
    const uint8_t* __restrict__ buf, long buf_len,
    const long* __restrict__ src_pos, const long* __restrict__ lengths,
    const long* __restrict__ out_offsets, long n, int chunk,
    uint8_t* __restrict__ out, long total_bytes) {
  __shared__ long s_off[kChunkMax];
  __shared__ long s_src[kChunkMax];
  __shared__ long s_ln[kChunkMax];

  const int tid = threadIdx.x;
  const long nchunks = (n + chunk - 1) / chunk;
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long v0 = c * chunk;
    const int cnt = (int)(n - v0 < chunk ? n - v0 : chunk);
    __syncthreads();     // the previous pass has read its tables out
    for (int i = tid; i < cnt; i += kBlock) {
      const long ln = lengths[v0 + i];
      s_off[i] = out_offsets[v0 + i];
      s_src[i] = src_pos[v0 + i];
      s_ln[i] = ln < 0 ? 0 : ln;
    }
    __syncthreads();
    // the chunk's output bytes [lo, hi), clipped to the output
    long lo = s_off[0];
    const long last = s_off[cnt - 1], last_ln = s_ln[cnt - 1];
    const long hi = last > total_bytes - last_ln ? total_bytes : last + last_ln;
    if (lo < 0) lo = 0;
    // blocks of 16 output bytes on 16-byte boundaries of `out`, one per lane
    for (long blk = (lo & ~15L) + (long)tid * 16; blk < hi; blk += kBlock * 16) {
      const long q0 = blk < lo ? lo : blk;
      int a = 0, b = cnt - 1;          // last value that starts at or below q0
      while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (s_off[m] <= q0) a = m; else b = m - 1;
      }
      // the block as two 64-bit halves, filled segment by segment: a
      // segment is the part of one value that lies in the block, at most 16
      // bytes, read as the aligned dwords around its source
      u64 acc0 = 0, acc1 = 0, have0 = 0, have1 = 0;
      const long q1 = blk + 16 < hi ? blk + 16 : hi;
      long q = q0;
      while (q < q1) {
        while (a + 1 < cnt && s_off[a + 1] <= q) ++a;
        const long r = q - s_off[a];
        const long ln = s_ln[a];
        if (r < 0 || r >= ln) {        // no value owns this byte
          ++q;
          continue;
        }
        const long rest = ln - r;
        const int b0 = (int)(q - blk);
        const int b1 = (int)(rest < q1 - q ? b0 + rest : q1 - blk);
        const long s = s_src[a] + r;   // source of byte b0
        u64 x0 = 0, x1 = 0;
        if (s >= 0 && s <= buf_len - (b1 - b0)) {
          const long base = s & ~3L;
          const int k = (int)(s & 3);
          const int need = (k + (b1 - b0) + 3) >> 2;   // 1..5 dwords
          uint32_t w[5];
#pragma unroll
          for (int i = 0; i < 5; ++i)
            w[i] = i < need && base + 4 * i + 4 <= buf_len
                       ? *(const uint32_t*)(buf + base + 4 * i) : 0u;
          // a segment that ends in the last, partial dword of `buf`
          if (base + 4 * need > buf_len) {
            const int i = (int)((buf_len - base) >> 2);
            uint32_t t = 0;
            for (long at = base + 4 * i; at < buf_len; ++at)
              t |= (uint32_t)buf[at] << (8 * (at & 3));
            if (i == 0) w[0] = t; else if (i == 1) w[1] = t;
            else if (i == 2) w[2] = t; else if (i == 3) w[3] = t; else w[4] = t;
          }
          const u64 t0 = w[0] | ((u64)w[1] << 32);
          const u64 t1 = w[2] | ((u64)w[3] << 32);
          const u64 t2 = w[4];
          x0 = k ? (t0 >> (8 * k)) | (t1 << (64 - 8 * k)) : t0;
          x1 = k ? (t1 >> (8 * k)) | (t2 << (64 - 8 * k)) : t1;
        } else {
          // the source leaves `buf`: byte by byte, outside reads as 0
          for (int i = 0; i < b1 - b0; ++i) {
            const long at = s + i;
            const u64 v = at >= 0 && at < buf_len ? buf[at] : 0;
            if (i < 8) x0 |= v << (8 * i); else x1 |= v << (8 * (i - 8));
          }
        }
        // move to byte b0 of the block and keep bytes [b0, b1)
        u64 y0, y1;
        if (b0 >= 8) {
          y0 = 0;
          y1 = x0 << (8 * (b0 - 8));
        } else {
          y0 = x0 << (8 * b0);
          y1 = b0 ? (x1 << (8 * b0)) | (x0 >> (64 - 8 * b0)) : x1;
        }
        const u64 m0 = low_bytes(b1 < 8 ? b1 : 8) & ~low_bytes(b0 < 8 ? b0 : 8);
        const u64 m1 = low_bytes(b1 > 8 ? b1 - 8 : 0) & ~low_bytes(b0 > 8 ? b0 - 8 : 0);
        acc0 |= y0 & m0;
        acc1 |= y1 & m1;
        have0 |= m0;
        have1 |= m1;
        q = blk + b1;
      }
      if ((have0 & have1) == ~0ull) {
        *(uint4*)(out + blk) =
            make_uint4((uint32_t)acc0, (uint32_t)(acc0 >> 32), (uint32_t)acc1,
                       (uint32_t)(acc1 >> 32));
      } else {                         // the ends of the chunk
        for (int i = 0; i < 8; ++i) {
          if (have0 >> (8 * i) & 1) out[blk + i] = (uint8_t)(acc0 >> (8 * i));
          if (have1 >> (8 * i) & 1) out[blk + 8 + i] = (uint8_t)(acc1 >> (8 * i));
        }
      }
    }
  }
}

void check_buf(const torch::Tensor& buf) {
  TORCH_CHECK(buf.scalar_type() == torch::kUInt8 && buf.is_contiguous(),
              "buf must be contiguous uint8");
}

void check_i64(const torch::Tensor& t, const torch::Tensor& buf, long n,
               const char* what) {
  TORCH_CHECK(t.scalar_type() == torch::kInt64 && t.dim() == 1 &&
                  t.is_contiguous() && t.size(0) == n,
              what, " must be contiguous int64 of one length");
  TORCH_CHECK(t.device() == buf.device(), what, " and buf on different devices");
}

}  // namespace

std::vector<torch::Tensor> pq_bytearray_index(torch::Tensor buf, torch::Tensor pages,
                                              int64_t total) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  check_buf(buf);
  TORCH_CHECK(pages.scalar_type() == torch::kInt64 && pages.dim() == 2 &&
                  pages.size(1) == 6 && pages.is_contiguous(),
              "pages must be contiguous int64 [n,6]");
  TORCH_CHECK(buf.device() == pages.device(), "buf and pages on different devices");
  TORCH_CHECK(total >= 0, "total must not be negative");
  long np = pages.size(0);
  TORCH_CHECK(np < (1L << 31), "too many pages");
  // zero-filled: a row no page owns reads as length 0 at position 0
  auto lengths = torch::zeros({total}, buf.options().dtype(torch::kInt64));
  auto src_pos = torch::zeros({total}, buf.options().dtype(torch::kInt64));
  auto status = torch::zeros({np}, buf.options().dtype(torch::kInt32));
  if (np == 0) return {lengths, src_pos, status};
  long groups = (np + kWaves - 1) / kWaves;
  if (groups > 8192) groups = 8192;
  hipLaunchKernelGGL(bytearray_index_kernel, dim3((int)groups), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), (long)buf.numel(),
                     pages.data_ptr<long>(), (int)np, lengths.data_ptr<long>(),
                     src_pos.data_ptr<long>(), status.data_ptr<int>(), (long)total);
  return {lengths, src_pos, status};
}

torch::Tensor pq_gather_bytes(torch::Tensor buf, torch::Tensor src_pos,
                              torch::Tensor lengths, torch::Tensor out_offsets,
                              int64_t total_bytes) {
  CHECK_DEV(buf); CHECK_DEV(src_pos); CHECK_DEV(lengths); CHECK_DEV(out_offsets);
  check_buf(buf);
  TORCH_CHECK(src_pos.dim() == 1, "src_pos must be one-dimensional");
  long n = src_pos.size(0);
  check_i64(src_pos, buf, n, "src_pos");
  check_i64(lengths, buf, n, "lengths");
  check_i64(out_offsets, buf, n, "out_offsets");
  TORCH_CHECK(total_bytes >= 0, "total_bytes must not be negative");
  auto out = torch::empty({total_bytes}, buf.options().dtype(torch::kUInt8));
  if (n == 0 || total_bytes == 0) return out;
  TORCH_CHECK(((size_t)out.data_ptr() & 15) == 0, "output must be 16-byte aligned");
  TORCH_CHECK(((size_t)buf.data_ptr() & 3) == 0, "buf must be 4-byte aligned");
  // chunks small enough to fill the chip, large enough to fill a workgroup
  long chunk = (n + 2047) / 2048;
  chunk = chunk < 32 ? 32 : (chunk > kChunkMax ? kChunkMax : chunk);
  long blocks = (n + chunk - 1) / chunk;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(gather_bytes_kernel, dim3((int)blocks), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), (long)buf.numel(),
                     src_pos.data_ptr<long>(), lengths.data_ptr<long>(),
                     out_offsets.data_ptr<long>(), n, (int)chunk,
                     out.data_ptr<uint8_t>(), (long)total_bytes);
  return out;
}
