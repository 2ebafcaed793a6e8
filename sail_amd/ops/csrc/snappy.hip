// Snappy page decompression (gfx950 / CDNA4).
//
// Parquet stores each page of a SNAPPY column chunk as one raw Snappy stream:
// a varint preamble (the uncompressed length) followed by literal and copy
// elements. pq_snappy_decompress expands a whole table of such pages in one
// launch, so that the page decoders of parquet_decode.hip can run on the
// result (datasource/gpu_parquet.py, opt-in via sail.io.gpu_snappy).
//
// Page descriptor: int64 [n,6] = {src_off, src_len, uncompressed_len, out_off,
// 0, 0}. One 256-thread workgroup owns one page (grid-stride over pages).
// Per batch, all threads stage the next kWin input bytes in LDS (the tag
// walk is a chain of dependent byte loads: from LDS each costs an LDS
// round trip, from global memory a cache or HBM one), thread 0 walks the
// tags of that window into two LDS tables (literals, copies) and validates
// every element; then all threads expand the batch:
//
//   1. literals read only the input, so they all copy in parallel (8 lanes
//      per short literal, the whole workgroup per long one);
//   2. copies are split by thread 0 into groups, in stream order. A copy
//      joins the open group when its source ends at or below the output
//      position where the group began, i.e. it reads only bytes that
//      literals, earlier groups or earlier batches wrote. A copy that
//      reads bytes of the group's latest copy A, all of them inside A and A
//      not overlapping itself, is pointed at A's own source instead
//      (src = A.src + (src - A.dst)) and joins too: this shortens the
//      copy-of-copy chains that sorted, repeated integers compress to
//      (TPC-H l_orderkey: 142 -> 100 ms of kernel time at SF1). Any other
//      copy opens a new group. The copies of one group run in parallel (8 lanes each,
//      byte i from src + i % period with period = the tag's offset, which
//      makes overlapping copies with offset < length correct), and a
//      __syncthreads() separates a group from the next, so a store and any
//      later load of the same byte are always on opposite sides of a
//      workgroup barrier.
//
// Throughput: the serial tag walk is the bound. Measured on an MI355X at
// about 0.4 us per element and page (a 1 MiB page of PLAIN int64 holds some
// 260,000 elements), 0.5 GB/s decompressed over a stock pyarrow TPC-H SF1
// lineitem file (profiles/README.md). Pages run in parallel, so files with
// many small pages fare better than files with few large ones.
//
// Status contract: status[p] == 0 exactly when the preamble equals
// uncompressed_len, the input is consumed exactly and exactly
// uncompressed_len bytes were produced. Otherwise the first problem met in
// stream order is reported and the page's output bytes are unspecified:
//
//   1  preamble missing its terminator within 5 bytes, or != uncompressed_len
//   2  input truncated: a tag's length/offset bytes or a literal's payload
//      run past src_len, or the input ends before uncompressed_len bytes
//      were produced (an empty input included)
//   3  output overrun: an element would produce more than uncompressed_len
//   4  bad copy offset: 0, or greater than the bytes produced so far
//   5  trailing input after uncompressed_len bytes were produced
//
// For one element the checks run in this order: header bytes present (2),
// then for a literal output room (3) before payload present (2); for a copy
// the offset (4) before output room (3).
//
// Bounds contract: for any page, well-formed or not, the kernel reads only
// buf[src_off, src_off+src_len) and writes only out[out_off,
// out_off+uncompressed_len); every element is validated before it enters a
// table. It terminates: each parsed element consumes at least one input byte
// and every loop is bounded by src_len or uncompressed_len. The host wrapper
// checks the table shape, that lengths are in [0, 2^31) and that every range
// lies inside its tensor.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be a device tensor")

namespace {

constexpr int kBlock = 256;     // 4 wave64
constexpr int kLits = 512;      // LDS literal-table entries per batch
constexpr int kCopies = 1024;   // LDS copy-table entries per batch
constexpr int kLanes = 8;       // lanes per short element
constexpr int kShort = 64;      // longest literal expanded by kLanes lanes
constexpr int kWin = 8192;      // input bytes staged in LDS per batch
constexpr int kTagMax = 5;      // longest element header: tag + 4 bytes

enum : int {
  kOk = 0,
  kPreamble = 1,
  kTruncated = 2,
  kOverrun = 3,
  kBadOffset = 4,
  kTrailing = 5,
};

__global__ __launch_bounds__(kBlock) void snappy_decompress_kernel(
    const uint8_t* __restrict__ buf, const long* __restrict__ pages, int npages,
    uint8_t* out, int* __restrict__ status) {
  __shared__ int l_dst[kLits], l_len[kLits], l_src[kLits];
  __shared__ int c_dst[kCopies], c_len[kCopies], c_src[kCopies], c_per[kCopies];
  __shared__ int g_start[kCopies + 1];  // copy-table index where group g begins
  __shared__ uint8_t s_in[kWin];
  __shared__ int s_pos, s_prod, s_nl, s_nc, s_ng, s_err, s_done;

  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    const long* pg = pages + (long)p * 6;
    const uint8_t* src = buf + pg[0];
    const int len = (int)pg[1];
    const int ulen = (int)pg[2];
    uint8_t* dst = out + pg[3];

    if (threadIdx.x == 0) {
      // preamble: at most 5 varint bytes, all inside the page
      int pos = 0, shift = 0, err = kOk;
      unsigned long long v = 0;
      bool closed = false;
      while (pos < len && shift <= 28) {
        uint8_t b = src[pos++];
        v |= (unsigned long long)(b & 0x7F) << shift;
        if (!(b & 0x80)) { closed = true; break; }
        shift += 7;
      }
      if (!closed) err = pos >= len && shift <= 28 ? kTruncated : kPreamble;
      else if (v != (unsigned long long)ulen) err = kPreamble;
      s_pos = pos;
      s_prod = 0;
      s_err = err;
    }
    __syncthreads();
    int wlo = s_pos;  // where the next batch's input window begins

    while (true) {
      // stage src[wlo, whi) in LDS; element headers are parsed from there
      const int whi = len - wlo < kWin ? len : wlo + kWin;
      for (int i = wlo + threadIdx.x; i < whi; i += kBlock) s_in[i - wlo] = src[i];
      __syncthreads();
      if (threadIdx.x == 0) {
        // win(i) == src[i] for wlo <= i < whi
        auto win = [&](int i) -> unsigned { return s_in[i - wlo]; };
        int nl = 0, nc = 0, ng = 0;
        int pos = s_pos, prod = s_prod, err = s_err;
        int group_lo = -1;  // output position where the open group began
        // the open group's latest copy, if it does not overlap itself
        int a_dst = 0, a_len = 0, a_src = 0;
        bool a_lin = false;
        // a header must lie inside the window, unless the window already
        // reaches the end of the input; then the checks against len hold
        while (err == kOk && nl < kLits && nc < kCopies && pos < len &&
               (whi == len || pos + kTagMax <= whi)) {
          if (prod == ulen) { err = kTrailing; break; }
          const unsigned tag = win(pos++);
          if ((tag & 3) == 0) {  // literal
            unsigned lm1 = tag >> 2;
            if (lm1 >= 60) {  // tags 60..63: 1..4 length bytes follow
              const int nb = (int)lm1 - 59;
              if (len - pos < nb) { err = kTruncated; break; }
              lm1 = 0;
              for (int i = 0; i < nb; ++i) lm1 |= (unsigned)win(pos + i) << (8 * i);
              pos += nb;
            }
            const long n = (long)lm1 + 1;
            if (n > (long)(ulen - prod)) { err = kOverrun; break; }
            if (n > (long)(len - pos)) { err = kTruncated; break; }
            l_dst[nl] = prod;
            l_len[nl] = (int)n;
            l_src[nl] = pos;
            ++nl;
            pos += (int)n;
            prod += (int)n;
          } else {  // copy with 1-, 2- or 4-byte offset
            const int kind = (int)(tag & 3);
            const int nb = kind == 1 ? 1 : (kind == 2 ? 2 : 4);
            if (len - pos < nb) { err = kTruncated; break; }
            int n;
            unsigned off;
            if (kind == 1) {
              n = 4 + (int)((tag >> 2) & 7);
              off = ((tag >> 5) << 8) | win(pos);
            } else {
              n = 1 + (int)(tag >> 2);
              off = 0;
              for (int i = 0; i < nb; ++i) off |= (unsigned)win(pos + i) << (8 * i);
            }
            pos += nb;
            if (off == 0 || off > (unsigned)prod) { err = kBadOffset; break; }
            if (n > ulen - prod) { err = kOverrun; break; }
            const int o = (int)off;
            const int m = n < o ? n : o;  // source bytes it reads
            int s = prod - o;
            if (group_lo < 0 || s + m > group_lo) {
              if (group_lo >= 0 && a_lin && s >= a_dst && s + m <= a_dst + a_len) {
                s = a_src + (s - a_dst);  // A's source: settled bytes
              } else {
                g_start[ng++] = nc;
                group_lo = prod;
              }
            }
            c_dst[nc] = prod;
            c_len[nc] = n;
            c_src[nc] = s;
            c_per[nc] = o;
            ++nc;
            a_dst = prod;
            a_len = n;
            a_src = s;
            a_lin = o >= n;
            prod += n;
          }
        }
        g_start[ng] = nc;
        // the input ended before the page was complete
        if (err == kOk && pos >= len && prod != ulen) err = kTruncated;
        s_nl = nl;
        s_nc = nc;
        s_ng = ng;
        s_pos = pos;
        s_prod = prod;
        s_err = err;
        s_done = (err != kOk || pos >= len) ? 1 : 0;
      }
      __syncthreads();
      // snapshot the shared loop state between the barriers (thread 0
      // rewrites it in the next parse phase); every thread takes the same
      // exit, error exit included. Elements already in the tables passed
      // validation, so expanding them stays inside the page.
      const int nl = s_nl;
      const int ng = s_ng;
      const int done = s_done;
      wlo = s_pos;

      // literals, short: kLanes lanes each
      for (int w = threadIdx.x; w < nl * kLanes; w += kBlock) {
        const int e = w / kLanes;
        const int n = l_len[e];
        if (n <= kShort) {
          const uint8_t* s = src + l_src[e];
          uint8_t* d = dst + l_dst[e];
          for (int i = w % kLanes; i < n; i += kLanes) d[i] = s[i];
        }
      }
      // literals, long: the whole workgroup each
      for (int e = 0; e < nl; ++e) {
        const int n = l_len[e];
        if (n > kShort) {
          const uint8_t* s = src + l_src[e];
          uint8_t* d = dst + l_dst[e];
          for (int i = threadIdx.x; i < n; i += kBlock) d[i] = s[i];
        }
      }
      __syncthreads();

      // copies: one barrier interval per group
      for (int g = 0; g < ng; ++g) {
        const int a = g_start[g];
        const int b = g_start[g + 1];
        for (int w = threadIdx.x; w < (b - a) * kLanes; w += kBlock) {
          const int e = a + w / kLanes;
          const int n = c_len[e];
          const int o = c_per[e];
          uint8_t* d = dst + c_dst[e];
          const uint8_t* s = dst + c_src[e];
          for (int i = w % kLanes; i < n; i += kLanes) d[i] = s[i < o ? i : i % o];
        }
        __syncthreads();
      }
      if (done) break;
    }
    if (threadIdx.x == 0) status[p] = s_err;
    __syncthreads();
  }
}

int grid_for(long npages) {
  long g = npages < 8192 ? npages : 8192;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

torch::Tensor pq_snappy_decompress(torch::Tensor buf, torch::Tensor pages,
                                   torch::Tensor out) {
  CHECK_DEV(buf); CHECK_DEV(pages); CHECK_DEV(out);
  TORCH_CHECK(buf.scalar_type() == torch::kUInt8 && buf.is_contiguous(),
              "buf must be contiguous uint8");
  TORCH_CHECK(out.scalar_type() == torch::kUInt8 && out.is_contiguous(),
              "out must be contiguous uint8");
  TORCH_CHECK(pages.scalar_type() == torch::kInt64 && pages.dim() == 2 &&
                  pages.size(1) == 6 && pages.is_contiguous(),
              "pages must be a contiguous int64 [n,6] table");
  int np = (int)pages.size(0);
  auto status = torch::empty({np}, buf.options().dtype(torch::kInt32));
  if (np == 0) return status;
  // the table is host-built and small: validate every range before a
  // kernel that trusts it runs
  auto host = pages.cpu();
  const int64_t* h = host.data_ptr<int64_t>();
  const int64_t lim = (int64_t)1 << 31;
  for (int p = 0; p < np; ++p) {
    const int64_t* r = h + (int64_t)p * 6;
    TORCH_CHECK(r[1] >= 0 && r[1] < lim, "page ", p, ": src_len ", r[1],
                " outside [0, 2^31)");
    TORCH_CHECK(r[2] >= 0 && r[2] < lim, "page ", p, ": uncompressed_len ",
                r[2], " outside [0, 2^31)");
    TORCH_CHECK(r[0] >= 0 && r[0] + r[1] <= buf.numel(), "page ", p,
                ": source range outside buf");
    TORCH_CHECK(r[3] >= 0 && r[3] + r[2] <= out.numel(), "page ", p,
                ": output range outside out");
  }
  hipLaunchKernelGGL(snappy_decompress_kernel, dim3(grid_for(np)), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), np,
                     out.data_ptr<uint8_t>(), status.data_ptr<int>());
  return status;
}
