// scan_reader.h: host half of the pipelined column-chunk reader.
//
// Plain C++17 and POSIX, no HIP and no torch, so it builds and is tested
// with the host compiler alone (tests/native/scan_reader_check.cpp). The
// device half (scan_reader.hip) gives it pinned slots and copies each slice
// to the device as it completes.
//
// A call turns a list of file ranges into the concatenation of their bytes,
// cut into slices of slice_bytes. Slices pass in order through a small ring
// of staging slots: a persistent pool of workers preads the pieces of a
// slice into its slot (pieces of at most task_bytes, so every worker helps
// on the earliest slice first), and the calling thread hands each finished
// slice to `consume` in output order. Before a slot is written again the
// caller's `wait_free(slot)` runs, which is where the device half waits for
// the copy that last left that slot.
//
// Guarantees: read() returns or throws only after every pread it queued has
// finished, so no worker writes into a slot afterwards; a worker error (a
// failed pread, end of file inside a range) reaches the caller as a
// std::runtime_error and leaves the reader usable; calls on one reader are
// serialised.
#pragma once

#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

namespace sail_io {

struct Range {
  int64_t start;
  int64_t end;
};

// part of a slice that is contiguous in the file
struct Piece {
  int64_t file_off;
  int64_t len;
  int64_t slot_off;
};

struct Slice {
  int64_t out_off = 0;
  int64_t len = 0;
  std::vector<Piece> pieces;
};

struct Config {
  int threads = 8;
  int64_t slice_bytes = 16 << 20;
  int slots = 8;
  int64_t task_bytes = 1 << 20;
};

inline int64_t env_int(const char* name, int64_t dflt, int64_t lo, int64_t hi) {
  const char* v = std::getenv(name);
  if (v == nullptr || *v == '\0') return dflt;
  char* end = nullptr;
  long long x = std::strtoll(v, &end, 10);
  if (end == v) return dflt;
  return std::min<int64_t>(std::max<int64_t>(x, lo), hi);
}

// SAIL_IO_READ_THREADS (8, at most 16: never sized by the machine's CPU
// count), SAIL_IO_READ_SLICE_BYTES (16 MiB), SAIL_IO_READ_SLOTS (8).
inline Config config_from_env() {
  Config c;
  c.threads = int(env_int("SAIL_IO_READ_THREADS", 8, 1, 16));
  c.slice_bytes = env_int("SAIL_IO_READ_SLICE_BYTES", 16 << 20, 1024, 256 << 20);
  c.slots = int(env_int("SAIL_IO_READ_SLOTS", 8, 2, 64));
  c.task_bytes = std::min<int64_t>(c.slice_bytes, 1 << 20);
  return c;
}

// Neighbours in the list that are also neighbours in the file become one
// range; empty ranges vanish. The concatenated bytes stay the same.
inline std::vector<Range> coalesce_ranges(const std::vector<Range>& in) {
  std::vector<Range> out;
  for (const Range& r : in) {
    if (r.start < 0 || r.end < r.start)
      throw std::invalid_argument("scan_reader: bad range");
    if (r.end == r.start) continue;
    if (!out.empty() && out.back().end == r.start)
      out.back().end = r.end;
    else
      out.push_back(r);
  }
  return out;
}

// A slice may hold parts of several ranges and a range may span several
// slices; a piece ends at a range end, a slice end or after task_bytes.
inline std::vector<Slice> make_slices(const std::vector<Range>& ranges,
                                      int64_t slice_bytes, int64_t task_bytes) {
  if (slice_bytes <= 0 || task_bytes <= 0)
    throw std::invalid_argument("scan_reader: slice and task sizes must be positive");
  std::vector<Slice> out;
  int64_t pos = 0;
  for (const Range& r : ranges) {
    if (r.start < 0 || r.end < r.start)
      throw std::invalid_argument("scan_reader: bad range");
    int64_t at = r.start;
    while (at < r.end) {
      if (out.empty() || out.back().len == slice_bytes) {
        out.emplace_back();
        out.back().out_off = pos;
      }
      Slice& s = out.back();
      int64_t n = std::min({r.end - at, slice_bytes - s.len, task_bytes});
      s.pieces.push_back(Piece{at, n, s.len});
      s.len += n;
      at += n;
      pos += n;
    }
  }
  return out;
}

class ScanReader {
 public:
  using AllocFn = std::function<void*(size_t)>;
  using FreeFn = std::function<void(void*)>;
  // wait_free(slot): returns once nothing reads the slot any more
  using WaitFreeFn = std::function<void(int)>;
  // consume(slot, data, out_off, len): slice bytes for [out_off, out_off+len)
  using ConsumeFn = std::function<void(int, const char*, int64_t, int64_t)>;

  explicit ScanReader(const Config& cfg, AllocFn alloc = nullptr, FreeFn free_fn = nullptr)
      : cfg_(cfg), free_(std::move(free_fn)) {
    if (cfg_.threads < 1 || cfg_.threads > 16)
      throw std::invalid_argument("scan_reader: 1 to 16 threads");
    if (cfg_.slots < 1 || cfg_.slice_bytes < 1 || cfg_.task_bytes < 1)
      throw std::invalid_argument("scan_reader: bad configuration");
    if (!alloc) {
      alloc = [](size_t n) { return std::malloc(n); };
      free_ = [](void* p) { std::free(p); };
    }
    for (int i = 0; i < cfg_.slots; ++i) {
      void* p = alloc(size_t(cfg_.slice_bytes));
      if (p == nullptr) {
        release_slots();
        throw std::bad_alloc();
      }
      slots_.push_back(static_cast<char*>(p));
    }
    for (int i = 0; i < cfg_.threads; ++i)
      workers_.emplace_back([this] { work(); });
  }

  ~ScanReader() { shutdown(); }
  ScanReader(const ScanReader&) = delete;
  ScanReader& operator=(const ScanReader&) = delete;

  const Config& config() const { return cfg_; }

  // Stops and joins the workers, closes the cached descriptors and frees
  // the slots. The caller makes sure nothing reads the slots any more.
  void shutdown() {
    std::lock_guard<std::mutex> call(call_mu_);
    {
      std::lock_guard<std::mutex> l(mu_);
      stop_ = true;
    }
    work_cv_.notify_all();
    for (std::thread& t : workers_)
      if (t.joinable()) t.join();
    workers_.clear();
    for (auto& kv : fds_) ::close(kv.second);
    fds_.clear();
    release_slots();
  }

  // Forget the cached descriptor of `path` (the file was replaced).
  void invalidate(const std::string& path) {
    std::lock_guard<std::mutex> call(call_mu_);
    auto it = fds_.find(path);
    if (it != fds_.end()) {
      ::close(it->second);
      fds_.erase(it);
    }
  }

  // Reads the concatenation of `ranges` of `path`, handing it to `consume`
  // slice by slice in output order. Returns the number of bytes.
  int64_t read(const std::string& path, const std::vector<Range>& ranges,
               const WaitFreeFn& wait_free, const ConsumeFn& consume) {
    std::lock_guard<std::mutex> call(call_mu_);
    if (workers_.empty()) throw std::runtime_error("scan_reader: reader is shut down");
    std::vector<Slice> slices =
        make_slices(coalesce_ranges(ranges), cfg_.slice_bytes, cfg_.task_bytes);
    const size_t n = slices.size();
    if (n == 0) return 0;
    const int fd = descriptor(path);
    const int nslots = int(slots_.size());
    CallState cs;
    cs.remaining.assign(n, 0);
    size_t submitted = 0;
    const size_t first = ring_pos_;
    ring_pos_ = (ring_pos_ + n) % size_t(nslots);
    try {
      for (size_t i = 0; i < n; ++i) {
        while (submitted < n && submitted < i + size_t(nslots)) {
          const int slot = int((first + submitted) % size_t(nslots));
          if (wait_free) wait_free(slot);
          submit(fd, slices[submitted], slots_[slot], &cs, submitted);
          ++submitted;
        }
        {
          std::unique_lock<std::mutex> l(mu_);
          done_cv_.wait(l, [&] { return cs.remaining[i] == 0; });
          if (cs.failed) throw std::runtime_error(cs.error);
        }
        const int slot = int((first + i) % size_t(nslots));
        consume(slot, slots_[slot], slices[i].out_off, slices[i].len);
      }
    } catch (...) {
      // queued pieces of this call are skipped, running ones finish: after
      // this no worker touches a slot on behalf of this call
      std::unique_lock<std::mutex> l(mu_);
      cs.failed = true;
      done_cv_.wait(l, [&] {
        for (size_t k = 0; k < submitted; ++k)
          if (cs.remaining[k] != 0) return false;
        return true;
      });
      throw;
    }
    return slices.back().out_off + slices.back().len;
  }

 private:
  struct CallState {
    std::vector<int> remaining;  // pieces of each slice not yet finished
    bool failed = false;
    std::string error;
  };

  struct Task {
    int fd;
    Piece piece;
    char* base;
    CallState* call;
    size_t slice;
  };

  void release_slots() {
    for (char* p : slots_)
      if (free_) free_(p);
    slots_.clear();
  }

  // one descriptor per path, opened once
  int descriptor(const std::string& path) {
    auto it = fds_.find(path);
    if (it != fds_.end()) return it->second;
    if (fds_.size() >= 256) {
      for (auto& kv : fds_) ::close(kv.second);
      fds_.clear();
    }
    int fd;
    do {
      fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    } while (fd < 0 && errno == EINTR);
    if (fd < 0)
      throw std::runtime_error("scan_reader: cannot open " + path + ": " +
                               std::strerror(errno));
    fds_[path] = fd;
    return fd;
  }

  void submit(int fd, const Slice& s, char* base, CallState* cs, size_t index) {
    {
      std::lock_guard<std::mutex> l(mu_);
      cs->remaining[index] = int(s.pieces.size());
      for (const Piece& p : s.pieces) queue_.push_back(Task{fd, p, base, cs, index});
    }
    work_cv_.notify_all();
  }

  // loops on short reads; end of file inside the piece is an error
  static std::string read_piece(int fd, const Piece& p, char* base) {
    int64_t got = 0;
    while (got < p.len) {
      ssize_t r = ::pread(fd, base + p.slot_off + got, size_t(p.len - got),
                          off_t(p.file_off + got));
      if (r < 0) {
        if (errno == EINTR) continue;
        return std::string("scan_reader: pread failed: ") + std::strerror(errno);
      }
      if (r == 0)
        return "scan_reader: end of file at offset " +
               std::to_string(p.file_off + got) + " inside a range";
      got += r;
    }
    return std::string();
  }

  void work() {
    std::unique_lock<std::mutex> l(mu_);
    for (;;) {
      work_cv_.wait(l, [&] { return stop_ || !queue_.empty(); });
      if (queue_.empty()) return;  // stop_ and nothing left to do
      Task t = queue_.front();
      queue_.pop_front();
      const bool skip = t.call->failed;
      l.unlock();
      std::string err;
      if (!skip) err = read_piece(t.fd, t.piece, t.base);
      l.lock();
      if (!err.empty() && !t.call->failed) {
        t.call->failed = true;
        t.call->error = err;
      }
      if (--t.call->remaining[t.slice] == 0) done_cv_.notify_all();
    }
  }

  Config cfg_;
  FreeFn free_;
  std::vector<char*> slots_;
  std::vector<std::thread> workers_;
  std::unordered_map<std::string, int> fds_;
  size_t ring_pos_ = 0;
  std::mutex call_mu_;  // one read() at a time; guards fds_ and ring_pos_
  std::mutex mu_;       // queue_, stop_ and every CallState
  std::condition_variable work_cv_;
  std::condition_variable done_cv_;
  std::deque<Task> queue_;
  bool stop_ = false;
};

}  // namespace sail_io
