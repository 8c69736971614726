"""CPU checks of the owners and the readback (csrc/swh_device.h): the header
compiled by a plain host compiler into a program with its own main and no
Python in the process, built once plainly and once with
-fsanitize=address,undefined. The program defines the HIP calls the header
uses as malloc-backed fakes that count what is live, refuse a handle that is
not live (a second free), log every call and can fail the k-th call. What the
counts, the statuses and the order of calls must be is stated here,
independently of the header."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "swift_subtask_dev_amd" / "csrc"
INCLUDE = ROOT / "include"

_MAIN = r"""
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "swh_device.h"

// ---- the fakes ------------------------------------------------------------
enum Kind { K_DEV = 0, K_PINNED, K_EVENT, K_STREAM, K_KINDS };
static std::set<void*>& live(int k) {
  static std::set<void*>* s = new std::set<void*>[K_KINDS];  // (never destroyed: no order issue)
  return s[k];
}
static std::vector<std::string>* g_log = new std::vector<std::string>();
static int g_calls = 0;    // the fallible calls so far
static int g_fail_at = 0;  // fail the k-th of them (0: none)
static std::string g_failed;

static void* take(int k, size_t bytes) {
  void* p = std::malloc(bytes ? bytes : 1);
  live(k).insert(p);
  return p;
}
static void give(int k, void* p, const char* what) {
  if (!live(k).erase(p)) {
    std::printf("FATAL %s of a handle that is not live\n", what);
    std::fflush(stdout);
    std::abort();
  }
  std::free(p);
}
// a fallible call: logged, counted, failed if it is the k-th
static bool fails(const char* name) {
  g_log->push_back(name);
  if (++g_calls != g_fail_at) return false;
  g_failed = name;
  return true;
}

extern "C" {
const char* hipGetErrorString(hipError_t) { return "fake"; }
hipError_t hipMalloc(void** p, size_t n) {
  if (fails("malloc")) return hipErrorOutOfMemory;
  *p = take(K_DEV, n);
  return hipSuccess;
}
hipError_t hipFree(void* p) { give(K_DEV, p, "hipFree"); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
  if (fails("hostmalloc")) return hipErrorOutOfMemory;
  *p = take(K_PINNED, n);
  return hipSuccess;
}
hipError_t hipHostFree(void* p) { give(K_PINNED, p, "hipHostFree"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  if (fails("eventcreate")) return hipErrorInvalidValue;
  *e = (hipEvent_t)take(K_EVENT, 1);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { give(K_EVENT, e, "hipEventDestroy"); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { give(K_STREAM, s, "hipStreamDestroy"); return hipSuccess; }
static void need_live(int k, void* p, const char* what) {
  if (!live(k).count(p)) {
    std::printf("FATAL %s on a handle that is not live\n", what);
    std::fflush(stdout);
    std::abort();
  }
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  need_live(K_EVENT, e, "record");
  need_live(K_STREAM, s, "record");
  return fails("record") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  need_live(K_EVENT, e, "sync");
  return fails("sync") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  need_live(K_EVENT, a, "elapsed");
  need_live(K_EVENT, b, "elapsed");
  if (fails("elapsed")) return hipErrorInvalidValue;
  *ms = 1.f;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  need_live(K_STREAM, s, "streamsync");
  return fails("streamsync") ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
  need_live(K_STREAM, st, "memcpy");
  if (fails("memcpy")) return hipErrorInvalidValue;
  std::memcpy(d, s, n);  // (the sanitized build checks both ranges)
  return hipSuccess;
}
}

namespace swh {
void set_error(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
}
}  // namespace swh
using namespace swh;

static void new_stream(Stream& s) { *s.put() = (hipStream_t)take(K_STREAM, 1); }

static void counts(const char* label) {
  std::printf("counts %s %zu %zu %zu %zu\n", label, live(K_DEV).size(), live(K_PINNED).size(),
              live(K_EVENT).size(), live(K_STREAM).size());
}
static void show_log(const char* label) {
  std::printf("log %s", label);
  for (const std::string& s : *g_log) std::printf(" %s", s.c_str());
  std::printf("\n");
  g_log->clear();
}

// ---- (d) copy traits ------------------------------------------------------
template <typename T>
constexpr bool move_only = !std::is_copy_constructible<T>::value &&
                           !std::is_copy_assignable<T>::value &&
                           std::is_nothrow_move_constructible<T>::value &&
                           std::is_nothrow_move_assignable<T>::value;
static_assert(move_only<DevBuf>, "DevBuf");
static_assert(move_only<HostBuf>, "HostBuf");
static_assert(move_only<Event>, "Event");
static_assert(move_only<Stream>, "Stream");
static_assert(move_only<Readback>, "Readback");
static_assert(!std::is_copy_constructible<StageTimer<3>>::value &&
              !std::is_copy_assignable<StageTimer<3>>::value, "StageTimer");

// ---- (a) moves and frees --------------------------------------------------
static int moves() {
  {
    Stream st;
    new_stream(st);
    DevBuf a, b;
    if (a.reserve(100) != SWH_OK || b.reserve(5000) != SWH_OK) return 1;
    std::printf("bytes %zu %zu\n", a.bytes, b.bytes);
    void* pa = a.ptr;
    if (a.reserve(50) != SWH_OK || a.ptr != pa) return 1;  // never shrinks, no new allocation
    counts("reserved");
    std::memset(a.ptr, 7, 100);
    if (a.grow_keep(300, 100, st) != SWH_OK) return 1;
    std::printf("grown %zu %d\n", a.bytes, (int)a.as<unsigned char>()[99]);
    counts("grown");
    DevBuf c(std::move(a));  // move-construct
    std::printf("moved_from %d %zu\n", (int)(a.ptr == nullptr), a.bytes);
    counts("move_constructed");
    b = std::move(c);  // move-assign onto a non-empty target: its buffer goes
    std::printf("moved_from %d %zu\n", (int)(c.ptr == nullptr), c.bytes);
    counts("move_assigned");
    std::swap(b, b);  // self-swap keeps the buffer
    std::printf("self_swapped %d %zu\n", (int)(b.ptr != nullptr), b.bytes);
    DevBuf d;
    if (d.reserve(64) != SWH_OK) return 1;
    void *pb = b.ptr, *pd = d.ptr;
    std::swap(b, d);
    std::printf("swapped %d\n", (int)(b.ptr == pd && d.ptr == pb));
    counts("swapped");
    HostBuf h, h2;
    if (h.reserve(10) != SWH_OK || h2.reserve(10000) != SWH_OK) return 1;
    std::printf("bytes %zu %zu\n", h.bytes, h2.bytes);
    HostBuf h3(std::move(h));
    h2 = std::move(h3);
    std::swap(h2, h2);
    counts("pinned_moved");
    Event e, e2;
    if (e.ensure() != SWH_OK || e.ensure() != SWH_OK || e2.ensure(hipEventDisableTiming) != SWH_OK)
      return 1;
    counts("events");
    Event e3(std::move(e));
    e2 = std::move(e3);
    std::swap(e2, e2);
    counts("events_moved");
    Stream st2(std::move(st));
    st = std::move(st2);
    Readback r, r2;
    if (r.prepare(32) != SWH_OK || r2.prepare(32) != SWH_OK) return 1;
    counts("readbacks");
    r2 = std::move(r);
    std::swap(r2, r2);
    counts("readback_moved");
  }
  counts("end");
  return 0;
}

// ---- (b) no leak on failure -----------------------------------------------
static swh_status sc_readback() {
  Stream st;
  new_stream(st);
  Readback r;
  SWH_TRY(r.prepare(64));
  SWH_TRY(r.queue(st));
  SWH_TRY(r.wait());
  return SWH_OK;
}
static swh_status sc_timer() {  // six events
  Stream st;
  new_stream(st);
  StageTimer<3> t;
  for (int k = 0; k < 3; k++) {
    SWH_TRY(t.begin(k, st));
    SWH_TRY(t.end(k, st));
  }
  float ms[3];
  SWH_TRY(t.read(ms));
  return SWH_OK;
}
static swh_status sc_grow() {
  Stream st;
  new_stream(st);
  DevBuf b;
  SWH_TRY(b.reserve(100));
  const swh_status s = b.grow_keep(1000, 100, st);
  // a failed grow keeps the old buffer
  if (s != SWH_OK && (b.ptr == nullptr || b.bytes != 256)) std::printf("FATAL grow lost its buffer\n");
  return s;
}
static int failures(const char* name, swh_status (*scenario)()) {
  g_calls = g_fail_at = 0;
  if (scenario() != SWH_OK) return 1;
  const int n = g_calls;
  std::printf("calls %s %d\n", name, n);
  counts(name);
  for (int k = 1; k <= n; k++) {
    g_calls = 0;
    g_fail_at = k;
    g_failed.clear();
    const swh_status s = scenario();
    std::printf("fail %s %d %s %d\n", name, k, g_failed.c_str(), (int)s);
    counts(name);
  }
  g_fail_at = 0;
  g_log->clear();
  return 0;
}

// ---- (c) the Readback state table -----------------------------------------
static void flags(const char* label, const Readback& r) {
  std::printf("flags %s %d %d\n", label, (int)r.pending, (int)r.has);
}
static int table() {
  Stream st;
  new_stream(st);
  {
    Readback r;
    if (r.wait() != SWH_OK) return 1;
    show_log("wait_first");
    flags("fresh", r);
    if (r.prepare(16) != SWH_OK) return 1;
    show_log("prepare");
    if (r.prepare(16) != SWH_OK || r.wait() != SWH_OK) return 1;
    show_log("prepare_again_wait");
    flags("prepared", r);
    r.dev<int>()[0] = 41;
    if (r.queue(st) != SWH_OK) return 1;
    r.dev<int>()[0] = 42;
    if (r.queue(st) != SWH_OK) return 1;
    flags("queued", r);
    if (r.wait() != SWH_OK) return 1;
    show_log("queue_queue_wait");
    flags("waited", r);
    std::printf("host %d\n", r.host<int>()[0]);
    if (r.wait() != SWH_OK) return 1;
    show_log("wait_again");
    flags("waited_again", r);
    const int src[4] = {1, 2, 3, 4};
    if (r.queue(st) != SWH_OK || r.set_host(src, sizeof(src)) != SWH_OK) return 1;
    show_log("queue_set_host");
    flags("set_host", r);
    std::printf("host %d %d\n", r.host<int>()[0], r.host<int>()[3]);
    if (r.queue(st) != SWH_OK) return 1;
    r.invalidate();
    flags("invalidated", r);
    if (r.wait() != SWH_OK) return 1;
    show_log("queue_invalidate_wait");
    if (r.mark(st) != SWH_OK) return 1;
    flags("marked", r);
    if (r.wait() != SWH_OK) return 1;
    show_log("mark_wait");
  }
  {
    Readback r;  // the empty-set path before any prepare: pinned memory alone
    if (r.set_host(nullptr, 24) != SWH_OK) return 1;
    show_log("set_host_first");
    flags("set_host_first", r);
    std::printf("host %d %d\n", r.host<int>()[0], r.host<int>()[5]);
    counts("set_host_first");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string m = argv[1];
  int r = 2;
  if (m == "moves") r = moves();
  if (m == "failures")
    r = failures("readback", sc_readback) | failures("timer", sc_timer) |
        failures("grow", sc_grow);
  if (m == "table") r = table();
  counts("exit");
  return r;
}
"""

SWH_OK, SWH_ERR_HIP, SWH_ERR_OOM = 0, 2, 7


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"
    d = tmp_path_factory.mktemp("device_" + request.param)
    src, exe = d / "device_main.cpp", d / "device_main"
    src.write_text(_MAIN)
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] \
        if request.param == "sanitized" else []
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-D__HIP_PLATFORM_AMD__",
                    f"-I{CSRC}", f"-I{INCLUDE}", "-isystem", str(rocm), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)

    def run(mode):
        p = subprocess.run([str(exe), mode], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout, p.stderr)
        assert "FATAL" not in p.stdout
        lines = [ln.split() for ln in p.stdout.splitlines()]
        assert lines[-1] == ["counts", "exit", "0", "0", "0", "0"]
        return lines[:-1]

    return run


def _counts(lines):
    """label -> every (device, pinned, events, streams) printed under it"""
    out = {}
    for ln in lines:
        if ln[0] == "counts":
            out.setdefault(ln[1], []).append(tuple(int(v) for v in ln[2:]))
    return out


def test_status_codes_are_the_abis():
    text = (INCLUDE / "swifthip.h").read_text()
    for name, value in (("SWH_OK", SWH_OK), ("SWH_ERR_HIP", SWH_ERR_HIP),
                        ("SWH_ERR_OOM", SWH_ERR_OOM)):
        assert f"{name} = {value}," in text, name


def test_moves_and_frees(program):
    lines = program("moves")
    c = _counts(lines)
    # (device, pinned, events, streams) live at each point of the scope
    assert c["reserved"] == [(2, 0, 0, 1)]
    assert c["grown"] == [(2, 0, 0, 1)]             # the old buffer went with the grow
    assert c["move_constructed"] == [(2, 0, 0, 1)]  # nothing made, nothing freed
    assert c["move_assigned"] == [(1, 0, 0, 1)]     # the target's own buffer was freed
    assert c["swapped"] == [(2, 0, 0, 1)]
    assert c["pinned_moved"] == [(2, 1, 0, 1)]
    assert c["events"] == [(2, 1, 2, 1)]            # a second ensure() makes nothing
    assert c["events_moved"] == [(2, 1, 1, 1)]
    assert c["readbacks"] == [(4, 3, 3, 1)]
    assert c["readback_moved"] == [(3, 2, 2, 1)]
    assert c["end"] == [(0, 0, 0, 0)]
    other = [ln for ln in lines if ln[0] != "counts"]
    assert other == [
        ["bytes", "256", "5000"],        # at least 256 bytes of device memory
        ["grown", "512", "7"],           # at least doubled, the used bytes kept
        ["moved_from", "1", "0"], ["moved_from", "1", "0"],
        ["self_swapped", "1", "512"],
        ["swapped", "1"],
        ["bytes", "4096", "10000"],      # at least a page of pinned memory
    ]


# the fallible HIP calls of each scenario, in order
SCENARIOS = {
    "readback": ["hostmalloc", "eventcreate", "malloc", "memcpy", "record", "sync"],
    "timer": ["eventcreate", "eventcreate", "record", "record"] * 3 + ["sync", "elapsed"] * 3,
    "grow": ["malloc", "malloc", "memcpy", "streamsync"],
}


def test_no_leak_on_failure(program):
    lines = program("failures")
    calls = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "calls"}
    assert calls == {name: len(seq) for name, seq in SCENARIOS.items()}
    fails = [ln[1:] for ln in lines if ln[0] == "fail"]
    assert len(fails) == sum(calls.values())
    seen = {name: [] for name in SCENARIOS}
    for name, k, failed, status in fails:
        assert failed == SCENARIOS[name][int(k) - 1], (name, k)
        want = SWH_ERR_OOM if failed in ("malloc", "hostmalloc") else SWH_ERR_HIP
        assert int(status) == want, (name, k, failed)
        seen[name].append(int(k))
    for name, ks in seen.items():
        assert ks == list(range(1, calls[name] + 1))
    for name, cs in _counts(lines).items():  # after every scope, failed or not
        assert len(cs) == calls[name] + 1
        assert set(cs) == {(0, 0, 0, 0)}, name


def test_readback_state_table(program):
    lines = program("table")
    logs = {ln[1]: ln[2:] for ln in lines if ln[0] == "log"}
    assert logs == {
        "wait_first": [],                                    # nothing queued: no call
        "prepare": ["hostmalloc", "eventcreate", "malloc"],
        "prepare_again_wait": [],                            # warm: no allocation
        "queue_queue_wait": ["memcpy", "record", "memcpy", "record", "sync"],  # one wait
        "wait_again": [],
        "queue_set_host": ["memcpy", "record", "sync"],      # the copy lands first
        "queue_invalidate_wait": ["memcpy", "record"],       # forgotten: nothing to wait for
        "mark_wait": ["record", "sync"],
        "set_host_first": ["hostmalloc"],
    }
    flags = {ln[1]: (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "flags"}
    assert flags == {  # (pending, has)
        "fresh": (0, 0), "prepared": (0, 0), "queued": (1, 1), "waited": (0, 1),
        "waited_again": (0, 1), "set_host": (0, 1), "invalidated": (0, 0), "marked": (1, 1),
        "set_host_first": (0, 1),
    }
    hosts = [ln[1:] for ln in lines if ln[0] == "host"]
    assert hosts == [["42"], ["1", "4"], ["0", "0"]]
    assert _counts(lines)["set_host_first"] == [(0, 1, 0, 1)]
