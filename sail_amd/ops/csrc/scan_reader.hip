// scan_reader.hip: device half of the pipelined column-chunk reader.
//
// pq_read_ranges(path, ranges, dst, copy_stream) moves the concatenation of
// the file ranges into the device tensor dst. The host half (scan_reader.h)
// preads slices into a fixed ring of pinned slots; as each slice completes,
// in order, it leaves for dst + offset with hipMemcpyAsync on the caller's
// copy stream and the slot's event is recorded. A slot goes back to the
// workers only once that event has completed, so the file read of later
// slices runs while earlier ones cross the link. The call returns when
// every copy has been issued; the caller orders its compute stream after
// the copy stream. The 16 zero bytes the page decoders may read past the
// payload are written with a memset on the same stream.
//
// The pinned footprint is slots x slice bytes (8 x 16 MiB by default),
// allocated once. Events persist between calls, so a later call waits for
// the copies of an earlier one before it reuses their slots. No kernel is
// launched here.
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "scan_reader.h"

namespace {

void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("scan_reader: ") + what + ": " +
                             hipGetErrorString(e));
}

struct DeviceRing {
  std::unique_ptr<sail_io::ScanReader> reader;
  std::vector<hipEvent_t> events;
  std::vector<char> pending;  // event recorded and not yet seen complete
  int device = -1;

  void wait_all() {
    for (size_t i = 0; i < events.size(); ++i)
      if (pending[i]) {
        (void)hipEventSynchronize(events[i]);
        pending[i] = 0;
      }
  }

  // returns once the copy that last left the slot is done
  void wait_slot(int slot) {
    if (size_t(slot) < pending.size() && pending[slot]) {
      hip_ok(hipEventSynchronize(events[slot]), "hipEventSynchronize");
      pending[slot] = 0;
    }
  }

  void drop_events() {
    wait_all();
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    events.clear();
    pending.clear();
  }

  // events belong to a device: made anew when the ring moves to another
  void bind(int dev) {
    if (dev == device && !events.empty()) return;
    drop_events();
    const int n = reader->config().slots;
    for (int i = 0; i < n; ++i) {
      hipEvent_t e;
      hip_ok(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
      events.push_back(e);
      pending.push_back(0);
    }
    device = dev;
  }

  ~DeviceRing() {
    // the slots must outlive the copies that read them
    drop_events();
    reader.reset();
  }
};

std::mutex g_mu;  // the ring, its events and its configuration
std::unique_ptr<DeviceRing> g_ring;
sail_io::Config g_cfg;
bool g_cfg_set = false;

DeviceRing& ring() {
  if (!g_ring) {
    if (!g_cfg_set) g_cfg = sail_io::config_from_env();
    auto r = std::make_unique<DeviceRing>();
    r->reader = std::make_unique<sail_io::ScanReader>(
        g_cfg,
        [](size_t n) -> void* {
          void* p = nullptr;
          if (hipHostMalloc(&p, n, hipHostMallocPortable) != hipSuccess) return nullptr;
          return p;
        },
        [](void* p) { (void)hipHostFree(p); });
    g_ring = std::move(r);
  }
  return *g_ring;
}

}  // namespace

int64_t pq_read_ranges(const std::string& path,
                       const std::vector<std::pair<int64_t, int64_t>>& ranges,
                       torch::Tensor dst, int64_t copy_stream) {
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == torch::kUInt8 && dst.is_contiguous(),
              "pq_read_ranges: dst must be a contiguous uint8 device tensor");
  std::vector<sail_io::Range> rs;
  rs.reserve(ranges.size());
  int64_t total = 0;
  for (const auto& r : ranges) {
    TORCH_CHECK(r.first >= 0 && r.second >= r.first, "pq_read_ranges: bad range");
    rs.push_back(sail_io::Range{r.first, r.second});
    total += r.second - r.first;
  }
  TORCH_CHECK(dst.numel() >= total + 16,
              "pq_read_ranges: dst holds ", dst.numel(), " bytes, needs ", total + 16);
  char* out = static_cast<char*>(dst.data_ptr());
  const int dev = int(dst.get_device());
  hipStream_t stream = reinterpret_cast<hipStream_t>(copy_stream);

  py::gil_scoped_release nogil;
  std::lock_guard<std::mutex> lock(g_mu);
  int prev = -1;
  hip_ok(hipGetDevice(&prev), "hipGetDevice");
  if (prev != dev) hip_ok(hipSetDevice(dev), "hipSetDevice");
  try {
    DeviceRing& rg = ring();
    rg.bind(dev);
    int64_t got = rg.reader->read(
        path, rs,
        [&rg](int slot) { rg.wait_slot(slot); },
        [&rg, out, stream](int slot, const char* data, int64_t off, int64_t len) {
          hip_ok(hipMemcpyAsync(out + off, data, size_t(len), hipMemcpyHostToDevice, stream),
                 "hipMemcpyAsync");
          // pending before the record is checked: a slot whose copy may have
          // been queued is never handed back without a wait
          rg.pending[slot] = 1;
          hip_ok(hipEventRecord(rg.events[slot], stream), "hipEventRecord");
        });
    if (got != total) throw std::runtime_error("scan_reader: byte count mismatch");
    hip_ok(hipMemsetAsync(out + total, 0, 16, stream), "hipMemsetAsync");
  } catch (...) {
    if (prev != dev) (void)hipSetDevice(prev);
    throw;
  }
  if (prev != dev) hip_ok(hipSetDevice(prev), "hipSetDevice");
  return total;
}

// The read half alone, for measurement (tools/upload_bench.py): the ranges
// pass through the ring and are dropped. Returns the number of bytes.
int64_t pq_reader_read_only(const std::string& path,
                            const std::vector<std::pair<int64_t, int64_t>>& ranges) {
  std::vector<sail_io::Range> rs;
  for (const auto& r : ranges) rs.push_back(sail_io::Range{r.first, r.second});
  py::gil_scoped_release nogil;
  std::lock_guard<std::mutex> lock(g_mu);
  DeviceRing& rg = ring();
  return rg.reader->read(
      path, rs, [&rg](int slot) { rg.wait_slot(slot); },
      [](int, const char*, int64_t, int64_t) {});
}

// threads, slice bytes and slots of the ring; a value of 0 takes the
// environment's (SAIL_IO_READ_THREADS, _SLICE_BYTES, _SLOTS). The ring is
// rebuilt on the next read, after the copies out of the old one are done.
void pq_reader_configure(int64_t threads, int64_t slice_bytes, int64_t slots) {
  sail_io::Config c = sail_io::config_from_env();
  if (threads > 0) c.threads = int(std::min<int64_t>(threads, 16));
  if (slice_bytes > 0) c.slice_bytes = std::min<int64_t>(slice_bytes, 256 << 20);
  if (slots > 0) c.slots = int(std::min<int64_t>(std::max<int64_t>(slots, 2), 64));
  c.task_bytes = std::min<int64_t>(c.slice_bytes, 1 << 20);
  py::gil_scoped_release nogil;
  std::lock_guard<std::mutex> lock(g_mu);
  g_ring.reset();
  g_cfg = c;
  g_cfg_set = threads > 0 || slice_bytes > 0 || slots > 0;
}

// (threads, slice bytes, slots, pinned bytes held now)
std::vector<int64_t> pq_reader_info() {
  std::lock_guard<std::mutex> lock(g_mu);
  sail_io::Config c = g_ring ? g_ring->reader->config()
                             : (g_cfg_set ? g_cfg : sail_io::config_from_env());
  return {c.threads, c.slice_bytes, c.slots,
          g_ring ? c.slice_bytes * c.slots : int64_t(0)};
}

void pq_reader_invalidate(const std::string& path) {
  std::lock_guard<std::mutex> lock(g_mu);
  if (g_ring) g_ring->reader->invalidate(path);
}

// Joins the workers and frees the ring; registered with atexit by the
// module so that interpreter exit never waits on a worker.
void pq_reader_shutdown() {
  py::gil_scoped_release nogil;
  std::lock_guard<std::mutex> lock(g_mu);
  g_ring.reset();
}
