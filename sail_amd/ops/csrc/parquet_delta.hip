// Fused DELTA_BINARY_PACKED decode (gfx950 / CDNA4): packed page bytes in,
// final int64 or int32 values out, one pass.
//
// pq_delta_decode + pq_segscan (parquet_decode.hip) zero-fill the output,
// write first-value-plus-deltas as int64, read that back for a per-page scan
// and, for INT32 columns, leave a cast to the caller. pq_delta_values reads
// the packed bytes once and writes each final value once.
//
// One 256-thread workgroup owns a page (grid-stride over the table) and
// works through it in tiles of up to 2048 deltas:
//   1. all threads stage a window of the page into LDS with 16-byte loads;
//   2. thread 0 walks the block headers in that window (LDS reads, not
//      dependent global loads). One lane runs this chain alone, so it does
//      the least it can per block: for a block of up to four miniblocks
//      that lies whole in the tile and the window it reads the header in
//      one round trip and records where the data starts, the four widths
//      and min_delta. Blocks cut by the window, by the page's end or by the
//      tile, and blocks of more miniblocks, get one table entry per
//      miniblock instead;
//   3. every thread unpacks 8 consecutive deltas. They never straddle a
//      miniblock (values per miniblock is a multiple of 8) and occupy `bw`
//      whole bytes, so the thread's segment is found by one division and
//      each value by aligned dword reads and a shift;
//   4. thread-local running sum, one wave scan of the thread totals with
//      __shfl_up, cross-wave carry through LDS;
//   5. the values go to LDS (over the window, which is spent by then) and
//      leave with 16-byte stores, each wave instruction covering 1 KiB of
//      contiguous output; the unaligned head and tail go element-wise.
// A tile ends early when the window runs out, even inside a miniblock; the
// next tile restages from there. Nothing outside [buf, buf + numel) is
// loaded and nothing outside a page's [out_row, out_row + n_values) stored.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be a device tensor")

namespace {

typedef unsigned long long u64;

constexpr int kBlock = 256;           // 4 wave64
constexpr int kGroup = 8;             // deltas per thread
constexpr int kTile = kBlock * kGroup;
// window: a full tile at width 64 (16 KiB) plus its block headers, the
// alignment slack and the step back to the current block's width bytes
constexpr int kWin = 17408;
constexpr int kWinMin = 2048;
constexpr int kBackStep = 1024;
constexpr int kSegs = 80;             // >= kBlock / 4 + 1 table entries
constexpr int kBlks = 64;             // whole blocks per tile: kBlock / 4

// Offsets within a page and the value count of a page are kept in 32 bits:
// parquet page headers carry both as i32. Longer descriptors are clipped.
constexpr long kPageMax = 0x7f000000L;

struct Walk {          // thread 0's place in the page; lives in LDS
  long min_delta;      // of the current block
  int pos;             // next block header, or the current miniblock's data
  int bw_at;           // the current block's bit-width bytes
  int didx;            // deltas handed out so far
  int mbpb;            // miniblocks per block
  int gps;             // 8-delta groups per miniblock
  int k;               // next miniblock of the block; == mbpb: header next
  int mb_g;            // groups already taken from the current miniblock
  int bw;              // its bit width
  unsigned bws;        // the block's width bytes when mbpb <= 4
};

template <typename T>
__global__ __launch_bounds__(kBlock) void delta_values_kernel(
    const uint8_t* __restrict__ buf, long buf_len,
    const long* __restrict__ pages, int npages, T* __restrict__ out,
    long total) {
  // window bytes in, tile values out; +32: unpack reads whole dwords up to
  // 11 bytes past a group's last byte
  __shared__ uint4 s_win4[(kWin + 32) / 16];
  __shared__ int seg_byte[kSegs];    // window offset of the segment's data
  __shared__ long seg_min[kSegs];
  __shared__ unsigned char seg_bw[kSegs];
  __shared__ u64 s_wtot[kBlock / 64];
  __shared__ Walk s_walk;
  __shared__ long s_first;
  __shared__ int s_ndeltas, s_next, s_g, s_f, s_end, s_gfast, s_gpb;
  // blocks that lie whole inside the tile and the window: thread 0 only
  // finds where each begins, the threads work out their miniblock
  __shared__ int blk_data[kBlks];    // window offset of the block's data
  __shared__ unsigned blk_bws[kBlks];
  __shared__ long blk_min[kBlks];

  uint8_t* win8 = (uint8_t*)s_win4;
  const uint32_t* win32 = (const uint32_t*)s_win4;
  T* obuf = (T*)s_win4;
  const int tid = threadIdx.x;

  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    const long* pgd = pages + (long)p * 6;
    const long src_off = pgd[0], src_len = pgd[1], out_row = pgd[3];
    const long aux = pgd[4];
    // a descriptor that points outside the buffer or the output is skipped
    // or clipped, never followed
    if (out_row < 0 || out_row > total || src_off < 0 || src_off > buf_len ||
        src_len < 0)
      continue;
    long nv = pgd[2];
    if (nv > total - out_row) nv = total - out_row;
    if (nv > kPageMax) nv = kPageMax;
    if (nv <= 0) continue;
    const int nvals = (int)nv;
    long pl = src_len < buf_len - src_off ? src_len : buf_len - src_off;
    const int page_len = (int)(pl < kPageMax ? pl : kPageMax);
    const uint8_t* src = buf + src_off;
    T* dst = out + out_row;

    // bytes one tile is expected to need, from the page's mean width
    long wl = ((long)page_len / nvals + 1) * (kTile + kTile / 4) + kBackStep + 256;
    const int want = (int)(wl < kWinMin ? kWinMin : (wl > kWin ? kWin : wl)) & ~15;

    int next = 0;       // page offset the next window has to cover
    int d0 = 0;         // deltas finished
    int ndeltas = 0;
    u64 carry = 0;
    bool first_tile = true;

    while (true) {
      // -- 1. stage [win_lo, win_hi) of the page from a 16-byte boundary --
      const int win_lo = next - (int)(((size_t)src + (size_t)next) & 15);
      const int win_hi = win_lo + want < page_len ? win_lo + want : page_len;
      // whole 16-byte pieces inside [buf, buf + buf_len) load as one
      const long lo_ok = -src_off, hi_ok = buf_len - src_off;   // page offsets
      for (int c = win_lo + tid * 16; c < win_hi; c += kBlock * 16) {
        uint4 v;
        if (c >= lo_ok && (long)c + 16 <= hi_ok) {
          v = *(const uint4*)(src + c);
        } else {
          uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (c + i >= lo_ok && c + i < hi_ok)
              q[i >> 2] |= (uint32_t)src[c + i] << (8 * (i & 3));
          v = make_uint4(q[0], q[1], q[2], q[3]);
        }
        s_win4[(c - win_lo) >> 4] = v;
      }
      __syncthreads();

      // -- 2. thread 0: page header once, then this tile's miniblocks ----
      if (tid == 0) {
        // header bytes come from the window; one outside it (a block's
        // width bytes far behind a huge miniblock) from global memory
        auto byte_at = [&](int q) -> unsigned {
          if (q >= win_lo && q < win_hi) return win8[q - win_lo];
          if (q >= 0 && q < page_len) return src[q];
          return 0u;
        };
        auto varint = [&](int& q) -> u64 {
          u64 v = 0;
          for (int sh = 0; sh < 70; sh += 7) {
            unsigned b = byte_at(q++);
            if (sh < 64) v |= (u64)(b & 0x7F) << sh;
            if (!(b & 0x80)) break;
          }
          return v;
        };
        auto zigzag = [](u64 v) -> long { return (long)(v >> 1) ^ -(long)(v & 1); };

        Walk w;
        int end = 0;
        bool parsed = false;
        if (first_tile) {
          int q = 0;
          const long block_size = (long)varint(q);
          const long mbpb = (long)varint(q);
          const long tot = (long)varint(q);
          s_first = zigzag(varint(q));
          const long n = tot < nvals ? tot : nvals;
          int nd = n > 0 ? (int)(n - 1) : 0;
          w.pos = q;
          w.bw_at = 0;
          w.min_delta = 0;
          w.didx = 0;
          w.mb_g = 0;
          w.bw = 0;
          w.bws = 0;
          // geometry the 8-delta groups cannot follow ends the page
          if (mbpb <= 0 || mbpb > (1 << 20) || block_size <= 0 ||
              block_size > (1L << 30) || block_size % mbpb != 0 ||
              (block_size / mbpb) % kGroup != 0) {
            nd = 0;
            w.mbpb = w.gps = 1;
          } else {
            w.mbpb = (int)mbpb;
            w.gps = (int)(block_size / mbpb / kGroup);
          }
          w.k = w.mbpb;
          s_ndeltas = nd;
          parsed = true;
        } else {
          w = s_walk;
        }
        const int nd = s_ndeltas;
        // whole blocks first (the common case, <= 4 miniblocks): per block
        // one header read and the sum of its widths
        int nblk = 0, gfast = 0, gpb = 1;
        if (w.mbpb <= 4 && w.gps <= kBlock && w.mb_g == 0) {
          gpb = w.mbpb * w.gps;
          while (w.k == w.mbpb && nblk < kBlks && gfast + gpb <= kBlock &&
                 nd - w.didx >= gpb * kGroup) {
            int q = w.pos;
            if (q < win_lo || q + 16 > win_hi) break;
            const uint32_t* d = win32 + ((q - win_lo) >> 2);
            const int sh = ((q - win_lo) & 3) * 8;
            const u64 a = d[0] | ((u64)d[1] << 32);
            const u64 b = d[2] | ((u64)d[3] << 32);
            const u64 c = d[4];
            const u64 lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
            const u64 hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
            u64 v = 0;
            int len = 0;
#pragma unroll
            for (int i = 0; i < 10; ++i) {
              const unsigned x =
                  (unsigned)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFF);
              if (7 * i < 64) v |= (u64)(x & 0x7F) << (7 * i);
              len = i + 1;
              if (!(x & 0x80)) break;
            }
            const unsigned bws =
                (unsigned)(len < 8 ? (lo >> (8 * len)) | (hi << (64 - 8 * len))
                                   : hi >> (8 * (len - 8)));
            int sum = 0;
            bool wide = false;
            for (int k = 0; k < w.mbpb; ++k) {
              const int bwk = (int)((bws >> (8 * k)) & 0xFF);
              wide |= bwk > 64;
              sum += bwk;
            }
            const int data = q + len + w.mbpb;
            const long nxt = (long)data + (long)w.gps * sum;
            if (wide || nxt > win_hi) break;    // left to the loop below
            blk_data[nblk] = data - win_lo;
            blk_bws[nblk] = bws;
            blk_min[nblk] = zigzag(v);
            ++nblk;
            gfast += gpb;
            w.didx += gpb * kGroup;
            w.pos = (int)nxt;
            parsed = true;
          }
        }
        int nseg = 0, g = gfast, f = 0;
        while (g < kBlock && w.didx < nd && nseg < kSegs) {
          if (w.mb_g == 0) {
            if (w.k == w.mbpb) {          // block header
              if (w.pos >= page_len) { end = 1; break; }
              if (g > 0 && win_hi < page_len &&
                  (long)w.pos + 10 + w.mbpb > win_hi)
                break;                    // let the next window hold it
              int q = w.pos;
              unsigned bws = 0;
              if (w.mbpb <= 4 && q >= win_lo && q + 16 <= win_hi) {
                // the usual header, up to 14 bytes, in one round trip to
                // LDS: five aligned dwords hold at least 17 bytes from q
                const uint32_t* d = win32 + ((q - win_lo) >> 2);
                const int sh = ((q - win_lo) & 3) * 8;
                const u64 a = d[0] | ((u64)d[1] << 32);
                const u64 b = d[2] | ((u64)d[3] << 32);
                const u64 c = d[4];
                const u64 lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
                const u64 hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
                u64 v = 0;
                int len = 0;
#pragma unroll
                for (int i = 0; i < 10; ++i) {
                  const unsigned x =
                      (unsigned)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFF);
                  if (7 * i < 64) v |= (u64)(x & 0x7F) << (7 * i);
                  len = i + 1;
                  if (!(x & 0x80)) break;
                }
                w.min_delta = zigzag(v);
                bws = (unsigned)(len < 8 ? (lo >> (8 * len)) | (hi << (64 - 8 * len))
                                         : hi >> (8 * (len - 8)));
                q += len;
              } else {
                w.min_delta = zigzag(varint(q));
                if (w.mbpb <= 4)
                  for (int k = 0; k < w.mbpb; ++k) bws |= byte_at(q + k) << (8 * k);
              }
              w.bws = bws;
              w.bw_at = q;
              w.pos = q + w.mbpb;         // < 2^31: both are far below it
              w.k = 0;
              parsed = true;
            }
            w.bw = w.mbpb <= 4 ? (int)((w.bws >> (8 * w.k)) & 0xFF)
                               : (int)byte_at(w.bw_at + w.k);
            if (w.bw > 64) { end = 1; break; }
          }
          const int rem = nd - w.didx;
          int need = (rem + kGroup - 1) / kGroup;
          if (need > w.gps - w.mb_g) need = w.gps - w.mb_g;
          const long data_at = (long)w.pos + (long)w.mb_g * w.bw;
          int fit = need;
          if (w.bw != 0 && (data_at < win_lo || data_at + (long)need * w.bw > win_hi))
            fit = data_at < win_lo || data_at >= win_hi
                      ? 0 : (int)(win_hi - data_at) / w.bw;
          int take = need < fit ? need : fit;
          if (take > kBlock - g) take = kBlock - g;
          if (take <= 0) break;
          seg_byte[nseg] = w.bw != 0 ? (int)(data_at - win_lo) : 0;
          seg_min[nseg] = w.min_delta;
          seg_bw[nseg] = (unsigned char)w.bw;
          if (nseg == 0) f = take;
          ++nseg;
          g += take;
          w.didx = rem <= take * kGroup ? nd : w.didx + take * kGroup;
          w.mb_g += take;
          if (w.mb_g == w.gps || w.didx >= nd) {
            // miniblocks are fully padded; past the page's end is all one
            long np_ = (long)w.pos + (long)w.gps * w.bw;
            w.pos = (int)(np_ < page_len ? np_ : page_len);
            w.mb_g = 0;
            ++w.k;
          }
          if (take < need && take == fit) break;   // window spent
        }
        // no group and no header in a whole window: the page is cut short
        if (g == 0 && !parsed) end = 1;
        // where the next window starts: the next byte needed, stepped back
        // to the block's width bytes when those are near
        long nb = (long)w.pos + (long)w.mb_g * w.bw;
        if (w.k < w.mbpb && w.bw_at <= nb && nb - w.bw_at <= kBackStep) nb = w.bw_at;
        if (nb >= page_len) {
          if (w.didx < nd && g == 0) end = 1;
          nb = 0;
        }
        s_walk = w;
        s_next = (int)nb;
        s_g = g;
        s_f = f;
        s_end = end;
        s_gfast = gfast;
        s_gpb = gpb;
      }
      __syncthreads();

      const int g = s_g, f = s_f, end = s_end, gfast = s_gfast;
      next = s_next;
      if (first_tile) {
        ndeltas = s_ndeltas;
        carry = (u64)s_first + (u64)aux;
        if (tid == 0) dst[0] = (T)carry;
        first_tile = false;
      }
      int cnt = g * kGroup;
      if (cnt > ndeltas - d0) cnt = ndeltas - d0;

      // -- 3. unpack this thread's 8 deltas; 4. scan ---------------------
      u64 v[kGroup];
#pragma unroll
      for (int i = 0; i < kGroup; ++i) v[i] = 0;
      if (tid < g) {
        const int gps = s_walk.gps;
        int bw, gb;
        u64 md;
        if (tid < gfast) {
          // group tid of the whole blocks: block, miniblock, group in it
          const int gpb = s_gpb;
          const int b = tid / gpb, r = tid - b * gpb;
          const int k = r / gps, j = r - k * gps;
          const unsigned bws = blk_bws[b];
          bw = (int)((bws >> (8 * k)) & 0xFF);
          const unsigned pre = k == 0 ? 0u : bws & (0xFFFFFFFFu >> (32 - 8 * k));
          const int before = (int)((pre & 0xFF) + ((pre >> 8) & 0xFF) + ((pre >> 16) & 0xFF));
          gb = blk_data[b] + gps * before + j * bw;
          md = (u64)blk_min[b];
        } else {
          const int t = tid - gfast;
          int s = 0, g0 = 0;
          if (t >= f) {
            s = 1 + (t - f) / gps;
            g0 = f + (s - 1) * gps;
          }
          bw = seg_bw[s];
          md = (u64)seg_min[s];
          gb = seg_byte[s] + (t - g0) * bw;
        }
        const u64 mask = bw >= 64 ? ~0ull : ((1ull << bw) - 1);
        const int dleft = cnt - tid * kGroup;   // valid deltas here
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
          u64 x = 0;
          if (bw != 0) {
            const int bit = i * bw;
            const int byte = gb + (bit >> 3);
            const int sh = (byte & 3) * 8 + (bit & 7);
            const uint32_t* q = win32 + (byte >> 2);
            x = (((u64)q[1] << 32) | q[0]) >> sh;
            if (bw > 33 && sh != 0) x |= (u64)q[2] << (64 - sh);
            x &= mask;
          }
          v[i] = i < dleft ? md + x : 0;
        }
      }
#pragma unroll
      for (int i = 1; i < kGroup; ++i) v[i] += v[i - 1];
      u64 incl = v[kGroup - 1];
      const int lane = tid & 63;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        u64 up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
      }
      if (lane == 63) s_wtot[tid >> 6] = incl;
      __syncthreads();     // wave totals in; every window read is done
      u64 base = carry + (incl - v[kGroup - 1]);
      u64 all = 0;
#pragma unroll
      for (int wv = 0; wv < kBlock / 64; ++wv) {
        u64 t = s_wtot[wv];
        if (wv < (tid >> 6)) base += t;
        all += t;
      }
      carry += all;

      // -- 5. values to LDS, then out in 16-byte pieces ------------------
      if (tid < g) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) obuf[tid * kGroup + i] = (T)(base + v[i]);
      }
      __syncthreads();
      {
        constexpr int per = 16 / (int)sizeof(T);
        const long e0 = out_row + 1 + d0;   // element of `out`
        const int head = (int)(e0 & (per - 1));
        // piece j of the tile holds tile values [j * per - head, + per)
        for (int j = tid; j * per - head < cnt; j += kBlock) {
          const int t0 = j * per - head;
          if (t0 >= 0 && t0 + per <= cnt) {
            T tmp[per];
#pragma unroll
            for (int e = 0; e < per; ++e) tmp[e] = obuf[t0 + e];
            uint4 pk;
            if constexpr (sizeof(T) == 8) {
              pk = make_uint4((uint32_t)(u64)tmp[0], (uint32_t)((u64)tmp[0] >> 32),
                              (uint32_t)(u64)tmp[1], (uint32_t)((u64)tmp[1] >> 32));
            } else {
              pk = make_uint4((uint32_t)tmp[0], (uint32_t)tmp[1],
                              (uint32_t)tmp[2], (uint32_t)tmp[3]);
            }
            *(uint4*)(out + (e0 + t0)) = pk;
          } else {
#pragma unroll
            for (int e = 0; e < per; ++e)
              if (t0 + e >= 0 && t0 + e < cnt) out[e0 + t0 + e] = obuf[t0 + e];
          }
        }
      }
      d0 += cnt;
      if (end || d0 >= ndeltas) break;
      __syncthreads();     // obuf read out before the window overwrites it
    }
    // a header count below n_values, or a page cut short: the rest of the
    // page's slots repeat the last value
    for (int i = 1 + d0 + tid; i < nvals; i += kBlock) dst[i] = (T)carry;
    __syncthreads();
  }
}

int grid_for(long npages) {
  long g = npages < 8192 ? npages : 8192;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

torch::Tensor pq_delta_values(torch::Tensor buf, torch::Tensor pages,
                              int64_t total, bool as_int32) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  TORCH_CHECK(buf.scalar_type() == torch::kUInt8 && buf.is_contiguous(),
              "buf must be contiguous uint8");
  TORCH_CHECK(pages.scalar_type() == torch::kInt64 && pages.dim() == 2 &&
                  pages.size(1) == 6 && pages.is_contiguous(),
              "pages must be contiguous int64 [n,6]");
  TORCH_CHECK(buf.device() == pages.device(), "buf and pages on different devices");
  TORCH_CHECK(total >= 0, "total must not be negative");
  long np = pages.size(0);
  TORCH_CHECK(np < (1L << 31), "too many pages");
  auto out = torch::empty({total}, buf.options().dtype(as_int32 ? torch::kInt32
                                                                : torch::kInt64));
  if (np == 0 || total == 0) return out;
  TORCH_CHECK(((size_t)out.data_ptr() & 15) == 0, "output must be 16-byte aligned");
  auto stream = hipStream_t(c10::hip::getCurrentHIPStream());
  if (as_int32) {
    hipLaunchKernelGGL(delta_values_kernel<int>, dim3(grid_for(np)), dim3(kBlock), 0,
                       stream, buf.data_ptr<uint8_t>(), (long)buf.numel(),
                       pages.data_ptr<long>(), (int)np, out.data_ptr<int>(),
                       (long)total);
  } else {
    hipLaunchKernelGGL(delta_values_kernel<long>, dim3(grid_for(np)), dim3(kBlock), 0,
                       stream, buf.data_ptr<uint8_t>(), (long)buf.numel(),
                       pages.data_ptr<long>(), (int)np, out.data_ptr<long>(),
                       (long)total);
  }
  return out;
}
