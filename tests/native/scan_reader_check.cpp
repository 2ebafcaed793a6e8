// Stand-alone check of sail_amd/ops/csrc/scan_reader.h (no GPU, no torch).
//
//   c++ -std=c++17 -O1 -g -pthread -I sail_amd/ops/csrc
//       tests/native/scan_reader_check.cpp -o scan_reader_check
//   ./scan_reader_check [work directory]
//
// Also meant to be built with -fsanitize=address,undefined and with
// -fsanitize=thread. Writes a file of about 100 KB of seeded bytes and reads
// range lists out of it through the reader with 4 KB slices, rings of 2 and
// 3 slots and 1, 2 and 8 threads; the expected bytes are always those of a
// plain sequential read. Prints one line per case and "ok" last; exits 1 on
// the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "scan_reader.h"

using sail_io::Config;
using sail_io::Range;
using sail_io::ScanReader;

namespace {

constexpr int64_t kFile = 100 * 1024 + 37;
constexpr int64_t kSlice = 4096;

int g_failed = 0;

void check(bool ok, const std::string& what) {
  if (!ok) {
    std::cout << "FAIL " << what << std::endl;
    g_failed = 1;
  }
}

std::vector<char> sequential(const std::string& path, const std::vector<Range>& ranges) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> out;
  for (const Range& r : ranges) {
    std::vector<char> part(size_t(r.end - r.start));
    f.seekg(r.start);
    f.read(part.data(), std::streamsize(part.size()));
    if (f.gcount() != std::streamsize(part.size())) {
      std::cout << "FAIL sequential read short" << std::endl;
      std::exit(1);
    }
    out.insert(out.end(), part.begin(), part.end());
  }
  return out;
}

// what the device half does with a slice, on the host: copy it out at once.
// The slot is poisoned afterwards, so a worker that wrote late, or a slice
// consumed twice, shows as wrong bytes.
struct Sink {
  std::vector<char> out;
  std::vector<int> slots_seen;
  int64_t next_off = 0;
  bool in_order = true;

  ScanReader::ConsumeFn fn() {
    return [this](int slot, const char* data, int64_t off, int64_t len) {
      if (off != next_off) in_order = false;
      next_off = off + len;
      if (int64_t(out.size()) < off + len) out.resize(size_t(off + len));
      std::memcpy(out.data() + off, data, size_t(len));
      std::memset(const_cast<char*>(data), 0xEE, size_t(len));
      slots_seen.push_back(slot);
    };
  }
};

bool read_matches(ScanReader& rd, const std::string& path, const std::vector<Range>& ranges,
                  const std::string& what, int* waits = nullptr) {
  Sink sink;
  int64_t n = rd.read(path, ranges, [&](int) { if (waits) ++*waits; }, sink.fn());
  std::vector<char> want = sequential(path, ranges);
  bool ok = n == int64_t(want.size()) && sink.out == want && sink.in_order;
  check(ok, what);
  return ok;
}

std::vector<Range> fifty_uneven(std::mt19937& rng) {
  std::vector<Range> rs;
  for (int i = 0; i < 50; ++i) {
    int64_t len;
    switch (i % 5) {
      case 0: len = 0; break;                        // zero-length
      case 1: len = 1 + int64_t(rng() % 100); break;  // far below a slice
      case 2: len = kSlice; break;
      case 3: len = 1 + int64_t(rng() % 3000); break;
      default: len = kSlice + 1 + int64_t(rng() % 6000); break;
    }
    int64_t start = int64_t(rng() % uint64_t(kFile - len));
    rs.push_back(Range{start, start + len});
  }
  return rs;
}

void run_cases(const std::string& path, int threads, int slots, int64_t task_bytes) {
  Config cfg;
  cfg.threads = threads;
  cfg.slice_bytes = kSlice;
  cfg.slots = slots;
  cfg.task_bytes = task_bytes;
  ScanReader rd(cfg);
  const std::string tag = " [threads " + std::to_string(threads) + ", slots " +
                          std::to_string(slots) + ", task " + std::to_string(task_bytes) + "]";
  std::mt19937 rng(1234u + unsigned(threads) * 16u + unsigned(slots));

  read_matches(rd, path, {{100, 9000}}, "single range" + tag);
  read_matches(rd, path, {}, "no ranges" + tag);
  read_matches(rd, path, {{500, 500}}, "one empty range" + tag);
  read_matches(rd, path, fifty_uneven(rng), "50 uneven ranges" + tag);
  read_matches(rd, path, {{7777, 7777 + 100}}, "range smaller than a slice" + tag);
  read_matches(rd, path, {{3, kFile}}, "range spanning many slices" + tag);
  read_matches(rd, path, {{10, 10 + 3 * kSlice}, {50000, 50000 + 2 * kSlice}},
               "total an exact multiple of the slice" + tag);
  read_matches(rd, path, {{10, 10 + 3 * kSlice}, {50000, 50000 + 2 * kSlice + 1}},
               "total one byte over a multiple" + tag);
  {
    // more slices than slots: the ring wraps and every slot is waited for
    int waits = 0;
    Sink sink;
    std::vector<Range> rs = {{0, 10 * kSlice + 5}};
    rd.read(path, rs, [&](int) { ++waits; }, sink.fn());
    check(sink.out == sequential(path, rs), "ring wraps: bytes" + tag);
    check(waits == 11 && int(sink.slots_seen.size()) == 11, "ring wraps: 11 slices" + tag);
    bool cyc = true;
    for (size_t i = 1; i < sink.slots_seen.size(); ++i)
      cyc = cyc && sink.slots_seen[i] == (sink.slots_seen[i - 1] + 1) % slots;
    check(cyc, "ring wraps: slots taken in rotation" + tag);
  }
  // two calls back to back on one reader
  read_matches(rd, path, {{1000, 30000}}, "back to back, first" + tag);
  read_matches(rd, path, {{20000, 61234}, {5, 4000}}, "back to back, second" + tag);
  {
    // a range ending past end of file: an error, not a hang
    bool threw = false;
    try {
      Sink sink;
      rd.read(path, {{0, 5000}, {kFile - 10000, kFile + 5000}}, nullptr, sink.fn());
    } catch (const std::runtime_error& e) {
      threw = std::string(e.what()).find("end of file") != std::string::npos;
    }
    check(threw, "range past end of file raises" + tag);
    read_matches(rd, path, {{kFile - 9000, kFile}}, "usable after the error" + tag);
  }
  {
    bool threw = false;
    try {
      Sink sink;
      rd.read(path + ".missing", {{0, 10}}, nullptr, sink.fn());
    } catch (const std::runtime_error&) {
      threw = true;
    }
    check(threw, "missing file raises" + tag);
    read_matches(rd, path, {{0, 100}}, "usable after a missing file" + tag);
  }
  {
    // an error raised by the consumer is passed on after the workers are quiet
    bool threw = false;
    int calls = 0;
    try {
      rd.read(path, {{0, 20 * kSlice}}, nullptr,
              [&](int, const char*, int64_t, int64_t) {
                if (++calls == 2) throw std::logic_error("consumer");
              });
    } catch (const std::logic_error&) {
      threw = true;
    }
    check(threw && calls == 2, "consumer error passed on" + tag);
    read_matches(rd, path, {{123, 45678}}, "usable after a consumer error" + tag);
  }
  {
    // adjacent ranges: coalesced and not coalesced give the same bytes
    std::vector<Range> split = {{100, 5000}, {5000, 5001}, {5001, 20000}, {20000, 20000},
                                {20000, 33333}, {40000, 41000}, {41000, 47000}};
    std::vector<Range> merged = sail_io::coalesce_ranges(split);
    check(merged.size() == 2 && merged[0].start == 100 && merged[0].end == 33333 &&
              merged[1].start == 40000 && merged[1].end == 47000,
          "coalesce_ranges merges neighbours" + tag);
    read_matches(rd, path, split, "adjacent ranges as given" + tag);
    read_matches(rd, path, merged, "adjacent ranges coalesced" + tag);
    check(sequential(path, split) == sequential(path, merged), "coalesced bytes equal" + tag);
    // neighbours in the file but not in the list must not be merged
    std::vector<Range> swapped = {{5000, 9000}, {100, 5000}};
    check(sail_io::coalesce_ranges(swapped).size() == 2, "order is kept" + tag);
    read_matches(rd, path, swapped, "ranges out of file order" + tag);
  }
  {
    // a replaced file is seen after invalidate()
    std::string p2 = path + ".swap";
    for (int round = 0; round < 2; ++round) {
      std::ofstream f(p2, std::ios::binary | std::ios::trunc);
      std::string body(9000, char('a' + round));
      f << body;
      f.close();
      rd.invalidate(p2);
      read_matches(rd, p2, {{0, 9000}}, "invalidate, round " + std::to_string(round) + tag);
    }
    std::remove(p2.c_str());
  }
  rd.shutdown();
  bool threw = false;
  try {
    Sink sink;
    rd.read(path, {{0, 10}}, nullptr, sink.fn());
  } catch (const std::runtime_error&) {
    threw = true;
  }
  check(threw, "read after shutdown raises" + tag);
  std::cout << (g_failed ? "failed" : "passed") << tag << std::endl;
}

void check_slicer() {
  auto s = sail_io::make_slices({{0, 10}, {100, 100 + 4096}, {9000, 9003}}, 4096, 1000);
  int64_t total = 0;
  bool ok = s.size() == 2 && s[0].len == 4096 && s[1].len == 13 && s[1].out_off == 4096;
  for (const auto& sl : s) {
    int64_t at = 0;
    for (const auto& p : sl.pieces) {
      ok = ok && p.slot_off == at && p.len > 0 && p.len <= 1000;
      at += p.len;
    }
    ok = ok && at == sl.len;
    total += sl.len;
  }
  check(ok && total == 10 + 4096 + 3, "make_slices layout");
  bool threw = false;
  try {
    sail_io::make_slices({{10, 5}}, 4096, 4096);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  check(threw, "make_slices rejects a reversed range");

  setenv("SAIL_IO_READ_THREADS", "64", 1);
  setenv("SAIL_IO_READ_SLICE_BYTES", "4096", 1);
  setenv("SAIL_IO_READ_SLOTS", "1", 1);
  Config c = sail_io::config_from_env();
  check(c.threads == 16 && c.slice_bytes == 4096 && c.slots == 2 && c.task_bytes == 4096,
        "config_from_env clamps");
  unsetenv("SAIL_IO_READ_THREADS");
  unsetenv("SAIL_IO_READ_SLICE_BYTES");
  unsetenv("SAIL_IO_READ_SLOTS");
  c = sail_io::config_from_env();
  check(c.threads == 8 && c.slice_bytes == (16 << 20) && c.slots == 8, "config_from_env defaults");
}

}  // namespace

int main(int argc, char** argv) {
  std::string dir = argc > 1 ? argv[1] : ".";
  std::string path = dir + "/scan_reader_check.bin";
  {
    std::mt19937 rng(20240607u);
    std::vector<char> bytes(static_cast<size_t>(kFile), 0);
    for (char& b : bytes) b = char(rng() & 0xFF);
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), std::streamsize(bytes.size()));
    if (!f) {
      std::cout << "FAIL cannot write " << path << std::endl;
      return 1;
    }
  }
  check_slicer();
  for (int slots : {2, 3})
    for (int threads : {1, 2, 8}) {
      run_cases(path, threads, slots, kSlice);
      if (g_failed) break;
    }
  // pieces smaller than a slice: several workers fill one slot
  if (!g_failed) run_cases(path, 8, 2, 1000);
  std::remove(path.c_str());
  if (g_failed) return 1;
  std::cout << "ok" << std::endl;
  return 0;
}
