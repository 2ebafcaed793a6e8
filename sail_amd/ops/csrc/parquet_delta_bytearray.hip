// DELTA_BYTE_ARRAY on the device (gfx950 / CDNA4): front-coded strings.
//
// A page's value region is <DELTA_BINARY_PACKED prefix lengths p[i]>
// <DELTA_BINARY_PACKED suffix lengths s[i]><suffix bytes>; value i is the
// first p[i] bytes of value i-1 followed by its s[i] suffix bytes, and the
// chain starts anew on every page. Both kernels give one wave a page and four
// pages a 256-thread workgroup, as pq_bytearray_index does: a page is a serial
// chain and a column has many pages. No workgroup barrier anywhere; the grid
// strides over the page table and a workgroup's spare waves fall through.
//
// pq_dba_lengths decodes the two length streams of every page. The streams are
// unvalidated file bytes, so this file has its own DELTA_BINARY_PACKED reader
// (pq_delta_decode trusts its header, its widths and its page length): every
// header byte is read through a bounds check, the geometry is checked, and a
// miniblock is unpacked only after the bytes it needs are known to lie in the
// page. The wave takes 64 values at a time: the block walk is wave-uniform,
// lane n unpacks delta n, one __shfl_up scan turns deltas into values. The
// second stream starts where the first ends, so the prefix lengths are decoded
// first and each lane reads its own back while the suffix lengths are decoded.
// Everything that can be said about a page without its bytes is checked here,
// so the offsets the host derives from `lengths` are sound:
//   1  a length stream is malformed or cut short (geometry, width > 64, a
//      header or a miniblock past the page)
//   2  a length is negative or does not fit 32 bits
//   3  the descriptor does not fit `buf` or the outputs (nothing is written)
//   4  p[0] != 0, or p[i] exceeds the length of value i-1
//   5  a value is longer than kMaxValue
//   6  the suffix bytes run past the page
//   7  the page's values leave its range of output bytes (pq_dba_expand)
//   8  a stream's value count differs from the page's n_values
// A page with a non-zero status has prefix, suffix and length 0 in all its rows.
//
// pq_dba_expand writes the values. Each wave keeps the *current value* in an
// LDS buffer of kMaxValue bytes and decodes in place: for value i bytes
// [0, p) are already right, the wave overwrites [p, p + s) with the suffix
// and stores [0, p + s) to out + offsets[i]. The prefix is never re-read from
// global memory and no lane reads an output byte.
//   - lane n loads (p, s, output offset) of value base + n for a batch of 64
//     and a wave scan of s gives its suffix position; the wave then steps
//     through the batch with that state in scalar registers (readlane), and
//     the lanes split the bytes of each value;
//   - the suffix bytes of a page are one contiguous run that does not depend
//     on the chain. They come through a per-wave LDS window of kWin bytes,
//     filled with 16-byte loads on 16-byte boundaries; the loads of the next
//     window are issued before this one is consumed and committed to LDS when
//     it is spent. A suffix may cross any number of window edges;
//   - the head of a value up to the first 16-byte boundary of `out` and the
//     tail after the last go out as one byte store (lanes 0-15 and 16-31), the
//     blocks between as 16-byte stores, each read from LDS as five dwords and
//     funnel-shifted. Nothing depends on how `out` is aligned;
//   - LDS traffic between lanes is ordered by wave_sync(): after a window is
//     committed, after the suffix is in the value buffer, after the value is
//     read out, and before a window is replaced.
// It repeats the checks above on what it is handed (they are scalar compares),
// so no tensor contents make it load outside `buf` or store outside the
// page's bytes [offsets[out_row], offsets[out_row + n_values)): a page that
// fails gets its status and zeroed `lengths` rows, and a page whose status is
// already non-zero is skipped.
//
// LDS: 4 x (kMaxValue + 16 + kWin) = 32832 bytes per workgroup, four workgroups
// per CU.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be a device tensor")

namespace {

typedef unsigned long long u64;

constexpr int kBlock = 256;              // 4 wave64
constexpr int kWaves = kBlock / 64;      // pages per workgroup
constexpr int kBatch = 64;               // values per batch: one per lane
constexpr int kMaxValue = 4096;          // longest value, bytes
constexpr int kWin = 4096;               // suffix staging window, bytes
constexpr int kPieces = kWin / 16 / 64;  // 16-byte loads per lane and window

// offsets within a page are kept in 32 bits, as in parquet_delta.hip
constexpr long kPageMax = 0x7f000000L;

enum : int {
  kBadStream = 1, kBadLength = 2, kBadDescriptor = 3, kBadPrefix = 4,
  kTooLong = 5, kSuffixPastPage = 6, kPastOutput = 7, kBadCount = 8
};

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

// lane k's copy of v, k wave-uniform
__device__ __forceinline__ int lane_i32(int v, int k) {
  return __builtin_amdgcn_readlane(v, k);
}

__device__ __forceinline__ long lane_i64(long v, int k) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)(u64)v, k);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)((u64)v >> 32), k);
  return (long)(((u64)hi << 32) | lo);
}

__device__ __forceinline__ long zigzag(u64 v) { return (long)(v >> 1) ^ -(long)(v & 1); }

// One page descriptor, checked against `buf` and the value outputs.
struct PageDesc {
  long src_off, src_len, nv, out_row;
  bool ok;
};

__device__ __forceinline__ PageDesc page_desc(const long* pages, long p, long buf_len,
                                              long total) {
  const long* pgd = pages + p * 6;
  PageDesc d;
  d.src_off = uniform(pgd[0]);
  d.src_len = uniform(pgd[1]);
  d.nv = uniform(pgd[2]);
  d.out_row = uniform(pgd[3]);
  d.ok = !(d.out_row < 0 || d.out_row > total || d.nv < 0 || d.nv > total - d.out_row ||
           d.nv > kPageMax || d.src_off < 0 || d.src_len < 0 || d.src_off > buf_len ||
           d.src_len > buf_len - d.src_off);
  return d;
}

// ---------------------------------------------------------------------------
// A DELTA_BINARY_PACKED stream inside [src, src + page_len), read by one wave.
// All of it is wave-uniform; nothing outside the page is ever loaded.
// ---------------------------------------------------------------------------
struct Stream {
  const uint8_t* src;
  int page_len;
  int pos;         // next header byte, or the current miniblock's data
  int mbpb, vpm;   // miniblocks per block, values per miniblock
  int k;           // next miniblock of the block; == mbpb: a block header is next
  int bw_at;       // the block's width bytes
  int bw;          // width of the current miniblock
  int left, used;  // its values not yet / already taken
  long min_delta;
  u64 last;        // the value before the next delta
  int st;
};

__device__ __forceinline__ unsigned stream_byte(Stream& S, int q) {
  if (q < 0 || q >= S.page_len) {
    S.st = kBadStream;
    return 0;
  }
  return __builtin_amdgcn_readfirstlane((unsigned)S.src[q]);
}

__device__ __forceinline__ u64 stream_varint(Stream& S) {
  u64 v = 0;
  for (int sh = 0; sh < 70; sh += 7) {
    const unsigned b = stream_byte(S, S.pos++);
    if (sh < 64) v |= (u64)(b & 0x7F) << sh;
    if (!(b & 0x80)) return v;
  }
  S.st = kBadStream;   // more than ten bytes
  return v;
}

__device__ __forceinline__ void stream_open(Stream& S, const uint8_t* src, int page_len,
                                            int start, int nvals) {
  S.src = src;
  S.page_len = page_len;
  S.pos = start;
  S.st = 0;
  S.mbpb = 1;
  S.vpm = 8;
  S.k = 1;
  S.bw_at = S.bw = S.left = S.used = 0;
  S.min_delta = 0;
  const u64 block = stream_varint(S);
  const u64 mbpb = stream_varint(S);
  const u64 count = stream_varint(S);
  S.last = (u64)zigzag(stream_varint(S));
  if (S.st != 0) return;
  if (mbpb == 0 || mbpb > 4096 || block == 0 || block > (1u << 20) || block % mbpb != 0 ||
      (block / mbpb) % 8 != 0) {
    S.st = kBadStream;
    return;
  }
  if (count != (u64)nvals) {
    S.st = kBadCount;
    return;
  }
  S.mbpb = (int)mbpb;
  S.vpm = (int)(block / mbpb);
  S.k = S.mbpb;
}

// `bw` bits at bit offset `bit` of src, 1 <= bw <= 64; the caller has checked
// that the bytes that hold them lie in the page
__device__ __forceinline__ u64 stream_bits(const uint8_t* src, long bit, int bw) {
  const long byte = bit >> 3;
  const int sh = (int)(bit & 7);
  const int need = (sh + bw + 7) >> 3;   // <= 9
  u64 lo = 0;
  for (int i = 0; i < 8; ++i)
    if (i < need) lo |= (u64)src[byte + i] << (8 * i);
  u64 v = lo >> sh;
  if (need > 8) v |= (u64)src[byte + 8] << (64 - sh);
  if (bw < 64) v &= (1ull << bw) - 1;
  return v;
}

// The next n <= 64 values of the stream: lane j < n gets value j of them. The
// stream's first value comes from its header, so the first batch takes one
// delta fewer. With S.st != 0 on return the values mean nothing.
__device__ __forceinline__ u64 stream_next(Stream& S, int lane, int n, bool first) {
  u64 d = 0;
  int filled = first ? 1 : 0;
  while (filled < n && S.st == 0) {
    if (S.left == 0) {
      if (S.k == S.mbpb) {
        S.min_delta = zigzag(stream_varint(S));
        if (S.st != 0 || S.mbpb > S.page_len - S.pos) {
          S.st = kBadStream;
          break;
        }
        S.bw_at = S.pos;
        S.pos += S.mbpb;
        S.k = 0;
      }
      S.bw = (int)stream_byte(S, S.bw_at + S.k);
      ++S.k;
      if (S.bw > 64) {
        S.st = kBadStream;
        break;
      }
      S.left = S.vpm;
      S.used = 0;
    }
    const int take = n - filled < S.left ? n - filled : S.left;
    const long need = ((long)(S.used + take) * S.bw + 7) >> 3;
    if (need > S.page_len - S.pos) {
      S.st = kBadStream;
      break;
    }
    if (lane >= filled && lane < filled + take) {
      u64 x = 0;
      if (S.bw != 0)
        x = stream_bits(S.src + S.pos, (long)(S.used + lane - filled) * S.bw, S.bw);
      d = (u64)S.min_delta + x;
    }
    filled += take;
    S.left -= take;
    S.used += take;
    if (S.left == 0) {   // miniblocks are padded to their full size
      const long np = (long)S.pos + (long)S.vpm * S.bw / 8;
      S.pos = (int)(np < S.page_len ? np : S.page_len);
    }
  }
  u64 incl = d;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const u64 up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  const u64 v = S.last + incl;
  S.last = (u64)lane_i64((long)v, 63);   // lanes >= n add nothing
  return v;
}

// where the stream's bytes end, once all its values are taken
__device__ __forceinline__ int stream_end(const Stream& S) {
  if (S.left == 0) return S.pos;
  const long np = (long)S.pos + (long)S.vpm * S.bw / 8;
  return (int)(np < S.page_len ? np : S.page_len);
}

__global__ __launch_bounds__(kBlock) void dba_lengths_kernel(
    const uint8_t* __restrict__ buf, long buf_len, const long* __restrict__ pages,
    int npages, int* prefix, int* __restrict__ suffix, long* __restrict__ lengths,
    long* __restrict__ suffix_start, int* __restrict__ status, long total) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

  for (long p = (long)blockIdx.x * kWaves + wave; p < npages;
       p += (long)gridDim.x * kWaves) {
    const PageDesc pd = page_desc(pages, p, buf_len, total);
    if (!pd.ok) {
      if (lane == 0) status[p] = kBadDescriptor;
      continue;
    }
    if (lane == 0) suffix_start[p] = pd.src_off;
    if (pd.nv == 0) continue;
    const int nvals = (int)pd.nv;
    const int page_len = (int)(pd.src_len < kPageMax ? pd.src_len : kPageMax);
    const uint8_t* src = buf + pd.src_off;
    int* dpre = prefix + pd.out_row;
    int* dsuf = suffix + pd.out_row;
    long* dlen = lengths + pd.out_row;

    Stream S;
    stream_open(S, src, page_len, 0, nvals);
    int st = S.st;
    for (int base = 0; base < nvals && st == 0; base += kBatch) {
      const int n = nvals - base < kBatch ? nvals - base : kBatch;
      const u64 v = stream_next(S, lane, n, base == 0);
      st = S.st;
      // a negative length wraps to a huge one
      if (st == 0 && __ballot(lane < n && v > 0x7fffffffull) != 0) st = kBadLength;
      if (st == 0 && lane < n) dpre[base + lane] = (int)v;
    }
    int end = 0;
    long sum_s = 0;      // suffix bytes of the page
    if (st == 0) {
      stream_open(S, src, page_len, stream_end(S), nvals);
      st = S.st;
      long prev_len = 0; // length of the value before the batch
      for (int base = 0; base < nvals && st == 0; base += kBatch) {
        const int n = nvals - base < kBatch ? nvals - base : kBatch;
        const u64 v = stream_next(S, lane, n, base == 0);
        st = S.st;
        if (st != 0) break;
        if (__ballot(lane < n && v > 0x7fffffffull) != 0) {
          st = kBadLength;
          break;
        }
        // the lane's own store of the first pass
        const long pre = lane < n ? dpre[base + lane] : 0;
        const long len = lane < n ? pre + (long)v : 0;
        long before = __shfl_up(len, 1);
        if (lane == 0) before = prev_len;
        if (__ballot(lane < n && pre > before) != 0) {
          st = kBadPrefix;
          break;
        }
        if (__ballot(len > kMaxValue) != 0) {
          st = kTooLong;
          break;
        }
        if (lane < n) {
          dsuf[base + lane] = (int)v;
          dlen[base + lane] = len;
        }
        prev_len = lane_i64(len, n - 1);
        int sum = lane < n ? (int)v : 0;   // <= 64 * kMaxValue
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        sum_s += __builtin_amdgcn_readfirstlane(sum);
      }
      if (st == 0) {
        end = stream_end(S);
        if (sum_s > (long)page_len - end) st = kSuffixPastPage;
      }
    }
    if (st != 0) {
      for (int i = lane; i < nvals; i += 64) {
        dpre[i] = 0;
        dsuf[i] = 0;
        dlen[i] = 0;
      }
      if (lane == 0) status[p] = st;
    } else if (lane == 0) {
      suffix_start[p] = pd.src_off + end;
    }
  }
}

// ---------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void dba_expand_kernel(
    const uint8_t* __restrict__ buf, long buf_len, const long* __restrict__ pages,
    int npages, const int* __restrict__ prefix, const int* __restrict__ suffix,
    const long* __restrict__ suffix_start, const long* __restrict__ offsets,
    long* __restrict__ lengths, int* status, long total, uint8_t* __restrict__ out,
    long out_len) {
  __shared__ uint4 s_cur[kWaves][(kMaxValue + 16) / 16];   // +16: the funnel's fifth dword
  __shared__ uint4 s_win[kWaves][kWin / 16];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* cur8 = (uint8_t*)s_cur[wave];
  const uint32_t* cur32 = (const uint32_t*)s_cur[wave];
  uint4* win4 = s_win[wave];
  const uint8_t* win8 = (const uint8_t*)s_win[wave];

  for (long p = (long)blockIdx.x * kWaves + wave; p < npages;
       p += (long)gridDim.x * kWaves) {
    if (__builtin_amdgcn_readfirstlane(status[p]) != 0) continue;
    const PageDesc pd = page_desc(pages, p, buf_len, total);
    if (!pd.ok) {
      if (lane == 0) status[p] = kBadDescriptor;
      continue;
    }
    if (pd.nv == 0) continue;
    const int nvals = (int)pd.nv;
    const int* dpre = prefix + pd.out_row;
    const int* dsuf = suffix + pd.out_row;
    const long* doff = offsets + pd.out_row;
    long* dlen = lengths + pd.out_row;

    int st = 0;
    // the suffix bytes: [ss, ss + region) of buf, inside the page
    const long ss = uniform(suffix_start[p]);
    const long out_lo = uniform(doff[0]), out_hi = uniform(doff[nvals]);
    if (ss < pd.src_off || ss > pd.src_off + pd.src_len) st = kBadDescriptor;
    else if (out_lo < 0 || out_hi < out_lo || out_hi > out_len) st = kPastOutput;
    const long rg = st != 0 ? 0 : pd.src_off + pd.src_len - ss;
    const int region = (int)(rg < kPageMax ? rg : kPageMax);
    // windows start on 16-byte boundaries of the address space: window k
    // holds suffix offsets [k * kWin - mis, (k + 1) * kWin - mis)
    const int mis = (int)((size_t)(buf + ss) & 15);

    // the 16-byte pieces of window k that hold suffix bytes, into registers
    auto fetch = [&](int k, uint4* r) {
#pragma unroll
      for (int j = 0; j < kPieces; ++j) {
        const long c = (long)k * kWin - mis + (j * 64 + lane) * 16;   // suffix offset
        uint4 v = make_uint4(0, 0, 0, 0);
        if (c < region) {
          const long a = ss + c;                                      // in buf
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
    auto commit = [&](const uint4* r) {
#pragma unroll
      for (int j = 0; j < kPieces; ++j) win4[j * 64 + lane] = r[j];
    };

    uint4 regs[kPieces];
    int hi = 0;          // the window in LDS
    int run = 0;         // suffix offset of the batch's first value
    int curlen = 0;      // length of the value in the buffer
    if (st == 0) {
      fetch(0, regs);
      commit(regs);
      fetch(1, regs);    // in flight while window 0 is consumed
      wave_sync();
    }
    for (int base = 0; base < nvals && st == 0; base += kBatch) {
      const int n = nvals - base < kBatch ? nvals - base : kBatch;
      int my_p = 0, my_s = 0;
      long my_off = 0;
      if (lane < n) {
        my_p = dpre[base + lane];
        my_s = dsuf[base + lane];
        my_off = doff[base + lane];
      }
      if (__ballot(my_p < 0 || my_s < 0) != 0) {
        st = kBadLength;
        break;
      }
      if (__ballot(my_p > kMaxValue || my_s > kMaxValue - my_p) != 0) {
        st = kTooLong;
        break;
      }
      int incl = my_s;   // <= 64 * kMaxValue
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
      }
      const int my_sp = incl - my_s;
      const int batch_bytes = lane_i32(incl, 63);
      if (batch_bytes > region - run) {
        st = kSuffixPastPage;
        break;
      }
      for (int k = 0; k < n; ++k) {
        const int pre = lane_i32(my_p, k), suf = lane_i32(my_s, k);
        const int len = pre + suf;
        const long off = lane_i64(my_off, k);
        if (pre > curlen) {
          st = kBadPrefix;
          break;
        }
        if (off < out_lo || off > out_hi - len) {
          st = kPastOutput;
          break;
        }
        // 1. the suffix into [pre, len) of the buffer, window by window
        int at = run + lane_i32(my_sp, k) + mis;   // in window coordinates
        int dst = pre, rem = suf;
        while (rem > 0) {
          const int wend = (hi + 1) * kWin;
          if (at >= wend) {   // this window is spent: bring in the next
            wave_sync();      // its reads are done before it is replaced
            ++hi;
            commit(regs);
            fetch(hi + 1, regs);
            wave_sync();
            continue;
          }
          const int take = rem < wend - at ? rem : wend - at;
          for (int j = lane; j < take; j += 64)
            cur8[dst + j] = win8[(at + j) & (kWin - 1)];
          at += take;
          dst += take;
          rem -= take;
        }
        wave_sync();          // the value is whole before it is read out
        // 2. [0, len) to out + off: head and tail by bytes, the 16-byte
        // blocks of `out` between them as one store each
        uint8_t* o = out + off;
        const int h0 = (int)((16 - ((size_t)o & 15)) & 15);
        const int h = h0 < len ? h0 : len;
        const int nb = (len - h) >> 4;
        const int t0 = h + (nb << 4);
        if (lane < 16) {
          if (lane < h) o[lane] = cur8[lane];
        } else if (lane < 32) {
          if (t0 + lane - 16 < len) o[t0 + lane - 16] = cur8[t0 + lane - 16];
        }
        const int sh = (h & 3) * 8;
        for (int b = lane; b < nb; b += 64) {
          const int c0 = h + (b << 4);
          const uint32_t* d = cur32 + (c0 >> 2);
          const u64 d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
          *(uint4*)(o + c0) = make_uint4((uint32_t)((d0 | (d1 << 32)) >> sh),
                                         (uint32_t)((d1 | (d2 << 32)) >> sh),
                                         (uint32_t)((d2 | (d3 << 32)) >> sh),
                                         (uint32_t)((d3 | (d4 << 32)) >> sh));
        }
        wave_sync();          // read out before the next value overwrites it
        curlen = len;
      }
      run += batch_bytes;
    }
    if (st != 0) {
      for (int i = lane; i < nvals; i += 64) dlen[i] = 0;
      if (lane == 0) status[p] = st;
    }
  }
}

void check_table(const torch::Tensor& buf, const torch::Tensor& pages) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  TORCH_CHECK(buf.scalar_type() == torch::kUInt8 && buf.is_contiguous(),
              "buf must be contiguous uint8");
  TORCH_CHECK(pages.scalar_type() == torch::kInt64 && pages.dim() == 2 &&
                  pages.size(1) == 6 && pages.is_contiguous(),
              "pages must be contiguous int64 [n,6]");
  TORCH_CHECK(buf.device() == pages.device(), "buf and pages on different devices");
  TORCH_CHECK(pages.size(0) < (1L << 31), "too many pages");
}

void check_vec(const torch::Tensor& t, const torch::Tensor& buf, c10::ScalarType dt,
               long n, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == buf.device(), what,
              " must be a device tensor on buf's device");
  TORCH_CHECK(t.scalar_type() == dt && t.dim() == 1 && t.is_contiguous() &&
                  t.size(0) == n,
              what, " has the wrong type, shape or length");
}

int groups_for(long np) {
  long g = (np + kWaves - 1) / kWaves;
  return (int)(g > 8192 ? 8192 : g);
}

}  // namespace

std::vector<torch::Tensor> pq_dba_lengths(torch::Tensor buf, torch::Tensor pages,
                                          int64_t total) {
  check_table(buf, pages);
  TORCH_CHECK(total >= 0, "total must not be negative");
  const long np = pages.size(0);
  // zero-filled: a row no page owns reads as an empty value
  auto i32 = buf.options().dtype(torch::kInt32);
  auto i64 = buf.options().dtype(torch::kInt64);
  auto prefix = torch::zeros({total}, i32);
  auto suffix = torch::zeros({total}, i32);
  auto lengths = torch::zeros({total}, i64);
  auto suffix_start = torch::zeros({np}, i64);
  auto status = torch::zeros({np}, i32);
  if (np != 0)
    hipLaunchKernelGGL(dba_lengths_kernel, dim3(groups_for(np)), dim3(kBlock), 0,
                       hipStream_t(c10::hip::getCurrentHIPStream()),
                       buf.data_ptr<uint8_t>(), (long)buf.numel(),
                       pages.data_ptr<long>(), (int)np, prefix.data_ptr<int>(),
                       suffix.data_ptr<int>(), lengths.data_ptr<long>(),
                       suffix_start.data_ptr<long>(), status.data_ptr<int>(),
                       (long)total);
  return {prefix, suffix, lengths, suffix_start, status};
}

void pq_dba_expand(torch::Tensor buf, torch::Tensor pages, torch::Tensor prefix,
                   torch::Tensor suffix, torch::Tensor suffix_start,
                   torch::Tensor offsets, torch::Tensor lengths, torch::Tensor status,
                   torch::Tensor out) {
  check_table(buf, pages);
  const long np = pages.size(0);
  TORCH_CHECK(lengths.dim() == 1, "lengths must be one-dimensional");
  const long total = lengths.size(0);
  check_vec(prefix, buf, torch::kInt32, total, "prefix");
  check_vec(suffix, buf, torch::kInt32, total, "suffix");
  check_vec(lengths, buf, torch::kInt64, total, "lengths");
  check_vec(offsets, buf, torch::kInt64, total + 1, "offsets");
  check_vec(suffix_start, buf, torch::kInt64, np, "suffix_start");
  check_vec(status, buf, torch::kInt32, np, "status");
  check_vec(out, buf, torch::kUInt8, out.dim() == 1 ? out.size(0) : -1, "out");
  if (np == 0) return;
  hipLaunchKernelGGL(dba_expand_kernel, dim3(groups_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), (long)buf.numel(), pages.data_ptr<long>(),
                     (int)np, prefix.data_ptr<int>(), suffix.data_ptr<int>(),
                     suffix_start.data_ptr<long>(), offsets.data_ptr<long>(),
                     lengths.data_ptr<long>(), status.data_ptr<int>(), total,
                     out.data_ptr<uint8_t>(), (long)out.numel());
}
