// GPU Parquet page decoders (gfx950 / CDNA4).
//
// The scan path the reference runs on arrow-rs's CPU reader
// (ref: crates/sail-data-source/src/formats/parquet/mod.rs) is re-designed
// here as batched device kernels: the host uploads raw column-chunk bytes
// to HBM, parses page headers (utils/thrift_compact.py), and launches ONE
// kernel per (column, encoding kind) over a page-descriptor table. Each
// workgroup (256 threads = 4 wave64) owns one page: lane 0 walks the
// sequential run/block headers into an LDS table, then all threads expand
// values in parallel (binary search over the LDS table). Fixed-width PLAIN
// regions are copied with funnel-shifted aligned dword loads so unaligned
// page payloads still move at near-memcpy rate.
//
// Encodings: PLAIN (fixed width + byte_array), RLE/bit-packed hybrid
// (definition levels, RLE_DICTIONARY indices), DELTA_BINARY_PACKED,
// DELTA_LENGTH_BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY decimals. PLAIN BOOLEAN,
// PLAIN INT96 and BYTE_STREAM_SPLIT are in parquet_types.hip; RLE booleans
// are hybrid runs of width 1 and use rle_decode_kernel. PLAIN byte_array
// pages and string dictionary pages go through parquet_bytearray.hip
// (pq_bytearray_index, pq_gather_bytes) unless sail.io.gpu_bytearray_fast
// is off; bytearray_walk_kernel and gather_strings_kernel below are the
// older pair. A string column that falls back from RLE_DICTIONARY to PLAIN
// pages is decoded from both kinds of page (datasource/gpu_parquet.py).
// The kernels see value and level regions only, so v1 and v2 data pages
// look the same to them (the host finds the regions). SNAPPY v1 pages are
// expanded first by snappy.hip when sail.io.gpu_snappy is on. Still on the
// host fallback (datasource/parquet_io.py): v2 pages in a compressed chunk,
// other codecs, DELTA_BYTE_ARRAY, BYTE_STREAM_SPLIT on FIXED_LEN_BYTE_ARRAY,
// nested columns.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <vector>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be a device tensor")

namespace {

constexpr int kBlock = 256;   // 4 wave64
constexpr int kRuns = 512;    // LDS run-table entries per batch

// Page descriptor: int64 [n,6] = {src_off, src_len, n_values, out_row, aux, bw}
//
// Buffer contract: `buf` is 4-byte aligned and extends at least 16 bytes past
// the end of the last page (the staging upload is total + 16 bytes).
// plain_copy_kernel and copy_bytes_kernel load whole aligned dwords, so they
// read the aligned dword that holds a page's last source byte, i.e. up to 3
// bytes before src_off and up to 3 bytes past src_off + src_len. Those bytes
// are read but never reach the output. A page with n_values == 0 writes
// nothing to any value output; delta_decode_kernel still writes data_end[p].
struct PageView {
  const uint8_t* src;
  long len;
  long nvals;
  long out_row;
  long aux;
  int bw;
};

__device__ __forceinline__ PageView page_view(const uint8_t* buf, const long* pages, int p) {
  const long* pg = pages + p * 6;
  return PageView{buf + pg[0], pg[1], pg[2], pg[3], pg[4], (int)pg[5]};
}

__device__ __forceinline__ unsigned long long read_varint(const uint8_t* src, long& pos) {
  unsigned long long out = 0;
  int shift = 0;
  while (true) {
    uint8_t b = src[pos++];
    out |= (unsigned long long)(b & 0x7F) << shift;
    if (!(b & 0x80)) return out;
    shift += 7;
  }
}

__device__ __forceinline__ long zigzag(unsigned long long v) {
  return (long)(v >> 1) ^ -(long)(v & 1);
}

// read `bw` bits at absolute bit offset `bit` (little-endian packing), bw<=64
__device__ __forceinline__ unsigned long long read_bits(const uint8_t* src, long bit, int bw) {
  long byte = bit >> 3;
  int sh = (int)(bit & 7);
  unsigned long long lo = 0;
  int need = (sh + bw + 7) >> 3;  // <= 9 bytes
  int nb = need < 8 ? need : 8;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < nb) lo |= (unsigned long long)src[byte + i] << (8 * i);
  unsigned long long v = lo >> sh;
  if (need > 8) {
    unsigned long long hi = src[byte + 8];
    v |= hi << (64 - sh);
  }
  if (bw < 64) v &= (1ull << bw) - 1;
  return v;
}

// ---------------------------------------------------------------------------
// RLE/bit-packed hybrid -> int32 (definition levels, dictionary indices)
// ---------------------------------------------------------------------------
__global__ void rle_decode_kernel(const uint8_t* __restrict__ buf,
                                  const long* __restrict__ pages, int npages,
                                  int* __restrict__ out) {
  __shared__ int r_start[kRuns];
  __shared__ int r_count[kRuns];
  __shared__ long r_payload[kRuns];  // RLE: value; packed: abs bit offset
  __shared__ char r_kind[kRuns];
  __shared__ long s_pos, s_vdone;
  __shared__ int s_nruns;

  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    PageView pg = page_view(buf, pages, p);
    int* dst = out + pg.out_row;
    if (threadIdx.x == 0) { s_pos = 0; s_vdone = 0; }
    __syncthreads();
    while (true) {
      if (threadIdx.x == 0) {
        int nr = 0;
        long pos = s_pos, vdone = s_vdone;
        while (nr < kRuns && vdone < pg.nvals && pos < pg.len) {
          unsigned long long h = read_varint(pg.src, pos);
          long cnt;
          if (h & 1) {  // bit-packed groups of 8
            long groups = (long)(h >> 1);
            cnt = groups * 8;
            if (cnt > pg.nvals - vdone) cnt = pg.nvals - vdone;
            r_kind[nr] = 1;
            r_payload[nr] = pos * 8;
            pos += groups * pg.bw;
          } else {  // RLE run, value in ceil(bw/8) LE bytes
            cnt = (long)(h >> 1);
            if (cnt > pg.nvals - vdone) cnt = pg.nvals - vdone;
            long v = 0;
            int nb = (pg.bw + 7) / 8;
            for (int i = 0; i < nb; ++i) v |= (long)pg.src[pos + i] << (8 * i);
            pos += nb;
            r_kind[nr] = 0;
            r_payload[nr] = v;
          }
          r_start[nr] = (int)vdone;
          r_count[nr] = (int)cnt;
          vdone += cnt;
          ++nr;
        }
        s_nruns = nr;
        s_pos = pos;
        s_vdone = vdone;
      }
      __syncthreads();
      // cache ALL shared loop state between the two barriers: thread 0
      // rewrites s_* in the next iteration's parse phase, so the exit
      // decision must be taken on locally-held copies (barrier-divergence
      // race found by the SF100 run — pages with >kRuns runs)
      int nr = s_nruns;
      long vdone_now = s_vdone;
      long pos_now = s_pos;
      if (nr != 0) {
        long lo = r_start[0];
        long hi = (long)r_start[nr - 1] + r_count[nr - 1];
        for (long v = lo + threadIdx.x; v < hi; v += blockDim.x) {
          int a = 0, b = nr - 1;
          while (a < b) {
            int mid = (a + b + 1) >> 1;
            if ((long)r_start[mid] <= v) a = mid; else b = mid - 1;
          }
          if (r_kind[a] == 0) {
            dst[v] = (int)r_payload[a];
          } else {
            long bit = r_payload[a] + (v - r_start[a]) * (long)pg.bw;
            dst[v] = (int)read_bits(pg.src, bit, pg.bw);
          }
        }
      }
      __syncthreads();
      if (nr == 0 || vdone_now >= pg.nvals || pos_now >= pg.len) break;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// PLAIN fixed-width copy: unaligned src -> W-aligned dst, funnel-shifted
// 32-bit loads (dst = out + out_row*W is 4-aligned for W in {4,8})
// ---------------------------------------------------------------------------
__global__ void plain_copy_kernel(const uint8_t* __restrict__ buf,
                                  const long* __restrict__ pages, int npages,
                                  uint8_t* __restrict__ out, int width) {
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    PageView pg = page_view(buf, pages, p);
    long total = pg.nvals * width;
    uint8_t* dst = out + pg.out_row * width;
    size_t srcaddr = (size_t)pg.src;
    const uint32_t* sa = (const uint32_t*)(srcaddr & ~(size_t)3);
    int sh = (int)(srcaddr & 3) * 8;
    long nwords = total >> 2;
    if (((size_t)dst & 3) == 0) {
      uint32_t* d32 = (uint32_t*)dst;
      if (sh == 0) {
        for (long i = threadIdx.x; i < nwords; i += blockDim.x) d32[i] = sa[i];
      } else {
        for (long i = threadIdx.x; i < nwords; i += blockDim.x)
          d32[i] = (sa[i] >> sh) | (sa[i + 1] << (32 - sh));
      }
      for (long i = (nwords << 2) + threadIdx.x; i < total; i += blockDim.x)
        dst[i] = pg.src[i];
    } else {
      for (long i = threadIdx.x; i < total; i += blockDim.x) dst[i] = pg.src[i];
    }
  }
}

// raw page-region copy into a byte blob at aux (DELTA_LENGTH payloads)
__global__ void copy_bytes_kernel(const uint8_t* __restrict__ buf,
                                  const long* __restrict__ pages, int npages,
                                  uint8_t* __restrict__ out) {
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    PageView pg = page_view(buf, pages, p);
    uint8_t* dst = out + pg.aux;
    size_t srcaddr = (size_t)pg.src;
    const uint32_t* sa = (const uint32_t*)(srcaddr & ~(size_t)3);
    int sh = (int)(srcaddr & 3) * 8;
    long nwords = pg.len >> 2;
    if (((size_t)dst & 3) == 0) {
      uint32_t* d32 = (uint32_t*)dst;
      if (sh == 0) {
        for (long i = threadIdx.x; i < nwords; i += blockDim.x) d32[i] = sa[i];
      } else {
        for (long i = threadIdx.x; i < nwords; i += blockDim.x)
          d32[i] = (sa[i] >> sh) | (sa[i + 1] << (32 - sh));
      }
      for (long i = (nwords << 2) + threadIdx.x; i < pg.len; i += blockDim.x)
        dst[i] = pg.src[i];
    } else {
      for (long i = threadIdx.x; i < pg.len; i += blockDim.x) dst[i] = pg.src[i];
    }
  }
}

// ---------------------------------------------------------------------------
// FIXED_LEN_BYTE_ARRAY big-endian signed -> int64 (parquet decimals)
// ---------------------------------------------------------------------------
__global__ void flba_i64_kernel(const uint8_t* __restrict__ buf,
                                const long* __restrict__ pages, int npages,
                                long* __restrict__ out, int width) {
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    PageView pg = page_view(buf, pages, p);
    long* dst = out + pg.out_row;
    for (long i = threadIdx.x; i < pg.nvals; i += blockDim.x) {
      const uint8_t* s = pg.src + i * width;
      long v = (s[0] & 0x80) ? -1 : 0;
      for (int b = 0; b < width; ++b) v = (v << 8) | s[b];
      dst[i] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// DELTA_BINARY_PACKED: writes delta contributions (first value at slot 0,
// min_delta+unpacked at slots 1..n-1); host finishes with a segmented
// cumulative sum. data_end[p] = byte offset where packed data ends.
// ---------------------------------------------------------------------------
__global__ void delta_decode_kernel(const uint8_t* __restrict__ buf,
                                    const long* __restrict__ pages, int npages,
                                    long* __restrict__ out,
                                    long* __restrict__ data_end) {
  __shared__ int m_base[kRuns];   // first delta index of miniblock
  __shared__ int m_cnt[kRuns];
  __shared__ long m_bit[kRuns];   // absolute bit offset of miniblock data
  __shared__ long m_min[kRuns];   // block min_delta
  __shared__ char m_bw[kRuns];
  __shared__ int s_nmb;
  __shared__ long s_pos, s_didx;
  __shared__ int s_vpm, s_mbpb;
  __shared__ long s_ndeltas;

  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    PageView pg = page_view(buf, pages, p);
    long* dst = out + pg.out_row;
    if (threadIdx.x == 0) {
      long pos = 0;
      long block_size = (long)read_varint(pg.src, pos);
      long mbpb = (long)read_varint(pg.src, pos);
      long total = (long)read_varint(pg.src, pos);
      long first = zigzag(read_varint(pg.src, pos));
      // a page with no non-null values owns no output slot: its out_row is
      // the next page's (or one past the end), so the store is predicated.
      // data_end[p] below is still the position just after the header.
      if (pg.nvals > 0) dst[0] = first;
      s_pos = pos;
      s_didx = 0;
      s_vpm = (int)(block_size / mbpb);
      s_mbpb = (int)mbpb;
      // total_count in the header; deltas = total-1 (clamped to page values)
      long n = total < pg.nvals ? total : pg.nvals;
      s_ndeltas = n > 0 ? n - 1 : 0;
    }
    __syncthreads();
    while (true) {
      if (threadIdx.x == 0) {
        int nmb = 0;
        long pos = s_pos, didx = s_didx;
        int vpm = s_vpm, mbpb = s_mbpb;
        long ndeltas = s_ndeltas;
        while (nmb + mbpb <= kRuns && didx < ndeltas && pos < pg.len) {
          long min_delta = zigzag(read_varint(pg.src, pos));
          long bw_at = pos;
          pos += mbpb;  // one bit-width byte per miniblock
          for (int k = 0; k < mbpb; ++k) {
            int bw = pg.src[bw_at + k];
            if (didx < ndeltas) {
              long cnt = ndeltas - didx < vpm ? ndeltas - didx : vpm;
              m_base[nmb] = (int)didx;
              m_cnt[nmb] = (int)cnt;
              m_bit[nmb] = pos * 8;
              m_min[nmb] = min_delta;
              m_bw[nmb] = (char)bw;
              ++nmb;
              didx += cnt;
              pos += (long)vpm * bw / 8;  // miniblocks fully padded
            }
            // trailing miniblocks with no values carry no data
          }
        }
        s_nmb = nmb;
        s_pos = pos;
        s_didx = didx;
      }
      __syncthreads();
      // same barrier-race discipline as rle_decode_kernel: take the exit
      // decision on copies cached between the two barriers
      int nmb = s_nmb;
      long didx_now = s_didx;
      long ndeltas_now = s_ndeltas;
      if (nmb != 0) {
        long lo = m_base[0];
        long hi = (long)m_base[nmb - 1] + m_cnt[nmb - 1];
        for (long d = lo + threadIdx.x; d < hi; d += blockDim.x) {
          int a = 0, b = nmb - 1;
          while (a < b) {
            int mid = (a + b + 1) >> 1;
            if ((long)m_base[mid] <= d) a = mid; else b = mid - 1;
          }
          int bw = m_bw[a];
          long v = bw == 0 ? 0
                           : (long)read_bits(pg.src, m_bit[a] + (d - m_base[a]) * (long)bw, bw);
          dst[1 + d] = m_min[a] + v;
        }
      }
      __syncthreads();
      if (nmb == 0 || didx_now >= ndeltas_now) break;
    }
    __syncthreads();
    if (threadIdx.x == 0) data_end[p] = s_pos;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Per-page inclusive scan (int64, in place, + per-page base from aux):
// finishes DELTA_BINARY_PACKED values (first+deltas -> values) and
// DELTA_LENGTH offsets entirely on device — replaces a whole-column
// torch.cumsum + cat + gather correction chain (was ~25% of decode GPU
// time in the SF100 profile).
// ---------------------------------------------------------------------------
constexpr int kScanTile = 2048;  // 256 threads x 8 elements

__global__ void segscan_kernel(long* __restrict__ data,
                               const long* __restrict__ pages, int npages) {
  __shared__ long tile[kScanTile];
  __shared__ long s_carry;
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    const long* pg = pages + p * 6;
    long n = pg[2];
    long* seg = data + pg[3];
    long base = pg[4];
    if (threadIdx.x == 0) s_carry = base;
    __syncthreads();
    for (long lo = 0; lo < n; lo += kScanTile) {
      int len = (int)((n - lo) < kScanTile ? (n - lo) : kScanTile);
      for (int i = threadIdx.x; i < len; i += blockDim.x)
        tile[i] = seg[lo + i];
      __syncthreads();
      // Hillis-Steele inclusive scan over the tile
      for (int off = 1; off < len; off <<= 1) {
        long vals[8];
        int cnt = 0;
        for (int i = threadIdx.x; i < len; i += blockDim.x)
          vals[cnt++] = (i >= off) ? tile[i - off] : 0;
        __syncthreads();
        cnt = 0;
        for (int i = threadIdx.x; i < len; i += blockDim.x)
          tile[i] += vals[cnt++];
        __syncthreads();
      }
      long carry = s_carry;
      for (int i = threadIdx.x; i < len; i += blockDim.x)
        seg[lo + i] = tile[i] + carry;
      __syncthreads();
      if (threadIdx.x == 0) s_carry = carry + tile[len - 1];
      __syncthreads();
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// PLAIN BYTE_ARRAY: sequential <u32 len><bytes> walk and one-thread-per-
// value copy. The older pair, kept behind sail.io.gpu_bytearray_fast=off:
// the walk checks no length against its page and leaves the rows of a
// truncated page unwritten (parquet_bytearray.hip does both)
// ---------------------------------------------------------------------------
__global__ void bytearray_walk_kernel(const uint8_t* __restrict__ buf,
                                      const long* __restrict__ pages, int npages,
                                      long* __restrict__ lengths,
                                      long* __restrict__ src_pos) {
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    PageView pg = page_view(buf, pages, p);
    if (threadIdx.x == 0) {
      long pos = 0;
      long base = (long)(pg.src - buf);
      for (long v = 0; v < pg.nvals && pos + 4 <= pg.len; ++v) {
        uint32_t ln = (uint32_t)pg.src[pos] | ((uint32_t)pg.src[pos + 1] << 8) |
                      ((uint32_t)pg.src[pos + 2] << 16) | ((uint32_t)pg.src[pos + 3] << 24);
        lengths[pg.out_row + v] = ln;
        src_pos[pg.out_row + v] = base + pos + 4;
        pos += 4 + ln;
      }
    }
  }
}

__global__ void gather_strings_kernel(const uint8_t* __restrict__ buf,
                                      const long* __restrict__ src_pos,
                                      const long* __restrict__ lengths,
                                      const long* __restrict__ out_offsets,
                                      long n, uint8_t* __restrict__ out) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = idx; i < n; i += stride) {
    const uint8_t* s = buf + src_pos[i];
    uint8_t* d = out + out_offsets[i];
    long ln = lengths[i];
    for (long b = 0; b < ln; ++b) d[b] = s[b];
  }
}

int grid_for(long npages) {
  long g = npages < 8192 ? npages : 8192;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

torch::Tensor pq_rle_decode(torch::Tensor buf, torch::Tensor pages, int64_t total) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  int np = (int)pages.size(0);
  auto out = torch::empty({total}, buf.options().dtype(torch::kInt32));
  if (np == 0 || total == 0) return out;
  hipLaunchKernelGGL(rle_decode_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     out.data_ptr<int>());
  return out;
}

torch::Tensor pq_plain_copy(torch::Tensor buf, torch::Tensor pages, int64_t total,
                            int64_t width) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  int np = (int)pages.size(0);
  auto out = torch::empty({total * width}, buf.options().dtype(torch::kUInt8));
  if (np == 0 || total == 0) return out;
  hipLaunchKernelGGL(plain_copy_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     out.data_ptr<uint8_t>(), (int)width);
  return out;
}

void pq_copy_bytes(torch::Tensor buf, torch::Tensor pages, torch::Tensor out) {
  CHECK_DEV(buf); CHECK_DEV(pages); CHECK_DEV(out);
  int np = (int)pages.size(0);
  if (np == 0) return;
  hipLaunchKernelGGL(copy_bytes_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     out.data_ptr<uint8_t>());
}

torch::Tensor pq_flba_i64(torch::Tensor buf, torch::Tensor pages, int64_t total,
                          int64_t width) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  TORCH_CHECK(width >= 1 && width <= 8, "flba width 1..8 supported");
  int np = (int)pages.size(0);
  auto out = torch::empty({total}, buf.options().dtype(torch::kInt64));
  if (np == 0 || total == 0) return out;
  hipLaunchKernelGGL(flba_i64_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     out.data_ptr<long>(), (int)width);
  return out;
}

std::vector<torch::Tensor> pq_delta_decode(torch::Tensor buf, torch::Tensor pages,
                                           int64_t total) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  int np = (int)pages.size(0);
  auto out = torch::zeros({total}, buf.options().dtype(torch::kInt64));
  auto data_end = torch::zeros({np}, buf.options().dtype(torch::kInt64));
  if (np == 0 || total == 0) return {out, data_end};
  hipLaunchKernelGGL(delta_decode_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     out.data_ptr<long>(), data_end.data_ptr<long>());
  return {out, data_end};
}

void pq_segscan(torch::Tensor data, torch::Tensor pages) {
  CHECK_DEV(data); CHECK_DEV(pages);
  int np = (int)pages.size(0);
  if (np == 0) return;
  hipLaunchKernelGGL(segscan_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     data.data_ptr<long>(), pages.data_ptr<long>(), np);
}

std::vector<torch::Tensor> pq_bytearray_walk(torch::Tensor buf, torch::Tensor pages,
                                             int64_t total) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  int np = (int)pages.size(0);
  auto lengths = torch::zeros({total}, buf.options().dtype(torch::kInt64));
  auto src_pos = torch::zeros({total}, buf.options().dtype(torch::kInt64));
  if (np == 0 || total == 0) return {lengths, src_pos};
  hipLaunchKernelGGL(bytearray_walk_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     lengths.data_ptr<long>(), src_pos.data_ptr<long>());
  return {lengths, src_pos};
}

torch::Tensor pq_gather_strings(torch::Tensor buf, torch::Tensor src_pos,
                                torch::Tensor lengths, torch::Tensor out_offsets,
                                int64_t total_bytes) {
  CHECK_DEV(buf); CHECK_DEV(src_pos); CHECK_DEV(lengths); CHECK_DEV(out_offsets);
  auto out = torch::empty({total_bytes}, buf.options().dtype(torch::kUInt8));
  long n = src_pos.size(0);
  if (n == 0 || total_bytes == 0) return out;
  long blocks = (n + kBlock - 1) / kBlock;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(gather_strings_kernel, dim3((int)blocks), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), src_pos.data_ptr<long>(),
                     lengths.data_ptr<long>(), out_offsets.data_ptr<long>(), n,
                     out.data_ptr<uint8_t>());
  return out;
}
