// GPU Parquet page decoders, second file (gfx950 / CDNA4): PLAIN BOOLEAN,
// PLAIN INT96 timestamps and BYTE_STREAM_SPLIT.
//
// Same conventions as parquet_decode.hip: one launch per (column, encoding
// kind) over a page-descriptor table, int64 [n,6] =
// {src_off, src_len, n_values, out_row, 0, 0}; a page with n_values == 0
// writes nothing; the output is allocated by the wrapper; launches go to the
// current stream. src_len is not read by these kernels: the host checks it
// against n_values before the table is uploaded (datasource/gpu_parquet.py:
// src_len*8 >= n for booleans, src_len >= 12n for INT96, src_len == width*n
// for BYTE_STREAM_SPLIT).
//
// None of the three needs a sequential walk, so there are no LDS tables: one
// thread per value, consecutive lanes on consecutive values. blockIdx.x
// strides over pages, blockIdx.y over 256-value slices of a page, so a file
// of few large pages still fills the device.
//
// Bytes read outside [src_off, src_off + src_len):
//   bool_unpack_kernel  none. Value i reads byte src_off + (i >> 3) only,
//                       and i < n_values <= 8 * src_len.
//   bss_decode_kernel   none. Value i reads bytes src_off + j*n_values + i,
//                       j < width, all below src_off + width*n_values.
//   int96_micros_kernel loads aligned dwords (buf is 4-byte aligned and
//                       extends 16 bytes past the last page, the contract of
//                       parquet_decode.hip). When src_off is a multiple of 4
//                       it reads nothing outside the page. Otherwise it reads
//                       the whole dwords that hold the first and the last
//                       byte of the page's values: up to 3 bytes before
//                       src_off and up to 3 bytes past src_off + 12*n_values.
//                       Those bytes are shifted out and never reach the
//                       output.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be a device tensor")

namespace {

constexpr int kBlock = 256;          // 4 wave64
constexpr long kMaxPageBlocks = 8192;
constexpr long kMaxSlices = 64;

// ---------------------------------------------------------------------------
// PLAIN BOOLEAN: bit i & 7 of src[i >> 3] -> one byte, 0 or 1. Eight lanes
// share a source byte (one broadcast load); a wave stores 64 consecutive
// bytes. out_row carries no alignment, so stores stay byte-sized. Padding
// bits of the last byte are never looked at: i < n_values.
// ---------------------------------------------------------------------------
__global__ void bool_unpack_kernel(const uint8_t* __restrict__ buf,
                                   const long* __restrict__ pages, int npages,
                                   uint8_t* __restrict__ out) {
  const long first = (long)blockIdx.y * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.y * blockDim.x;
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    const long* pg = pages + (long)p * 6;
    const uint8_t* src = buf + pg[0];
    const long n = pg[2];
    uint8_t* dst = out + pg[3];
    for (long i = first; i < n; i += step)
      dst[i] = (uint8_t)((src[i >> 3] >> (i & 7)) & 1);
  }
}

// ---------------------------------------------------------------------------
// PLAIN INT96 -> int64 microseconds since the Unix epoch. Value i is 12 bytes
// at src + 12*i: nanoseconds of day (LE int64), Julian day (LE int32). 12*i
// keeps the page's alignment mod 4 for every value, so the shift is uniform
// over the page: three aligned dwords when it is 0, four funnel-shifted ones
// otherwise. The division truncates (C++), the rest wraps in 64 bits.
// ---------------------------------------------------------------------------
__global__ void int96_micros_kernel(const uint8_t* __restrict__ buf,
                                    const long* __restrict__ pages, int npages,
                                    long* __restrict__ out) {
  const long first = (long)blockIdx.y * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.y * blockDim.x;
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    const long* pg = pages + (long)p * 6;
    const long n = pg[2];
    long* dst = out + pg[3];
    size_t srcaddr = (size_t)(buf + pg[0]);
    const uint32_t* sa = (const uint32_t*)(srcaddr & ~(size_t)3);
    const int sh = (int)(srcaddr & 3) * 8;
    for (long i = first; i < n; i += step) {
      const uint32_t* w = sa + 3 * i;
      uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      if (sh != 0) {
        uint32_t w3 = w[3];
        w0 = (w0 >> sh) | (w1 << (32 - sh));
        w1 = (w1 >> sh) | (w2 << (32 - sh));
        w2 = (w2 >> sh) | (w3 << (32 - sh));
      }
      long nanos = (long)(((unsigned long long)w1 << 32) | w0);
      long days = (long)(int)w2 - 2440588L;   // Julian day of 1970-01-01
      unsigned long long us = (unsigned long long)days * 86400000000ull +
                              (unsigned long long)(nanos / 1000);
      dst[i] = (long)us;
    }
  }
}

// ---------------------------------------------------------------------------
// BYTE_STREAM_SPLIT: byte j of value i is src[j*n + i]. Each of the W stream
// reads is coalesced over the wave (64 consecutive bytes); the value is put
// together in registers and stored once, naturally aligned (out is a tensor
// base plus a multiple of W).
// ---------------------------------------------------------------------------
template <int W, typename T>
__global__ void bss_decode_kernel(const uint8_t* __restrict__ buf,
                                  const long* __restrict__ pages, int npages,
                                  T* __restrict__ out) {
  const long first = (long)blockIdx.y * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.y * blockDim.x;
  for (int p = blockIdx.x; p < npages; p += gridDim.x) {
    const long* pg = pages + (long)p * 6;
    const uint8_t* src = buf + pg[0];
    const long n = pg[2];
    T* dst = out + pg[3];
    for (long i = first; i < n; i += step) {
      T v = 0;
#pragma unroll
      for (int j = 0; j < W; ++j) v |= (T)src[(long)j * n + i] << (8 * j);
      dst[i] = v;
    }
  }
}

void check_args(const torch::Tensor& buf, const torch::Tensor& pages, int64_t total) {
  CHECK_DEV(buf); CHECK_DEV(pages);
  TORCH_CHECK(buf.scalar_type() == torch::kUInt8 && buf.is_contiguous(),
              "buf must be contiguous uint8");
  TORCH_CHECK(pages.scalar_type() == torch::kInt64 && pages.dim() == 2 &&
                  pages.size(1) == 6 && pages.is_contiguous(),
              "pages must be contiguous int64 [n,6]");
  TORCH_CHECK(buf.device() == pages.device(), "buf and pages on different devices");
  TORCH_CHECK(total >= 0, "total must not be negative");
}

// x: pages (grid-stride past the cap); y: slices of a page, sized for the
// mean page so that small pages do not launch idle blocks
dim3 grid_for(long npages, long total) {
  long gx = npages < kMaxPageBlocks ? npages : kMaxPageBlocks;
  long mean = (total + npages - 1) / npages;
  long gy = (mean + 8 * kBlock - 1) / (8 * kBlock);   // ~8 values per thread
  gy = gy < 1 ? 1 : (gy > kMaxSlices ? kMaxSlices : gy);
  return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

torch::Tensor pq_bool_unpack(torch::Tensor buf, torch::Tensor pages, int64_t total) {
  check_args(buf, pages, total);
  long np = pages.size(0);
  auto out = torch::empty({total}, buf.options().dtype(torch::kUInt8));
  if (np == 0 || total == 0) return out;
  hipLaunchKernelGGL(bool_unpack_kernel, grid_for(np, total), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), (int)np,
                     out.data_ptr<uint8_t>());
  return out;
}

torch::Tensor pq_int96_micros(torch::Tensor buf, torch::Tensor pages, int64_t total) {
  check_args(buf, pages, total);
  long np = pages.size(0);
  auto out = torch::empty({total}, buf.options().dtype(torch::kInt64));
  if (np == 0 || total == 0) return out;
  TORCH_CHECK(((size_t)buf.data_ptr<uint8_t>() & 3) == 0, "buf must be 4-byte aligned");
  hipLaunchKernelGGL(int96_micros_kernel, grid_for(np, total), dim3(kBlock), 0,
                     hipStream_t(c10::hip::getCurrentHIPStream()),
                     buf.data_ptr<uint8_t>(), pages.data_ptr<long>(), (int)np,
                     out.data_ptr<long>());
  return out;
}

torch::Tensor pq_bss_decode(torch::Tensor buf, torch::Tensor pages, int64_t total,
                            int64_t width) {
  check_args(buf, pages, total);
  TORCH_CHECK(width == 4 || width == 8, "byte_stream_split width must be 4 or 8, got ",
              width);
  long np = pages.size(0);
  auto out = torch::empty({total * width}, buf.options().dtype(torch::kUInt8));
  if (np == 0 || total == 0) return out;
  auto stream = hipStream_t(c10::hip::getCurrentHIPStream());
  if (width == 4) {
    hipLaunchKernelGGL((bss_decode_kernel<4, uint32_t>), grid_for(np, total),
                       dim3(kBlock), 0, stream, buf.data_ptr<uint8_t>(),
                       pages.data_ptr<long>(), (int)np,
                       (uint32_t*)out.data_ptr<uint8_t>());
  } else {
    hipLaunchKernelGGL((bss_decode_kernel<8, unsigned long long>), grid_for(np, total),
                       dim3(kBlock), 0, stream, buf.data_ptr<uint8_t>(),
                       pages.data_ptr<long>(), (int)np,
                       (unsigned long long*)out.data_ptr<uint8_t>());
  }
  return out;
}
