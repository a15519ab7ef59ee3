"""Host check of csrc/side_worker.hpp, the parked thread of the time loops and the handle that owns its one job in flight, compiled with g++
into a stand-alone program (no GPU, no HIP).  The program checks, each as a numbered case that prints "ok <name>":

  run        a job runs, wait() returns, the handle is empty afterwards (and a second wait() is a no-op)
  throw      a job that throws makes wait() rethrow; the next job is unaffected
  dtor       a handle destroyed with its job in flight joins it (the job's writes to a stack variable of the owner are complete when the
             destructor returns) and swallows its error: the next job's wait() does not see it
  order      a second submit() while the first job blocks on a condition starts only after the first ended
  unjoined   the error of a job whose handle was overwritten by the next submission's surfaces at the next wait()
  move       moving a handle transfers ownership: one join (the source is empty, the target joins), move assignment joins what it replaces
  rounds     1000 submit / wait rounds on one worker; a worker destroyed while idle, one never used, one destroyed behind a finished job

The program is built and run three times: plain, with -fsanitize=address,undefined and with -fsanitize=thread; every run must exit 0 with all
cases reported and nothing on stderr."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")

SRC = r"""
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include "side_worker.hpp"

using dre::SideWorker;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static void nap(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }
static std::string what_of(SideWorker::Job& j) {
    try { j.wait(); } catch (const std::exception& e) { return e.what(); }
    return "";
}

static void case_run() {
    SideWorker w;
    int x = 0;
    SideWorker::Job j = w.submit([&x] { x = 7; });
    CHECK(j.pending());
    j.wait();
    CHECK(x == 7 && !j.pending() && !w.pending());
    j.wait();                                            // empty handle: nothing to do
    SideWorker::Job none;
    CHECK(!none.pending());
    none.wait(); none.reset();
    std::printf("ok run\n");
}

static void case_throw() {
    SideWorker w;
    SideWorker::Job j = w.submit([] { throw std::runtime_error("first"); });
    CHECK(what_of(j) == "first" && !j.pending());
    int x = 0;
    j = w.submit([&x] { x = 1; });
    CHECK(what_of(j).empty() && x == 1);
    std::printf("ok throw\n");
}

static void case_dtor() {
    SideWorker w;
    int owner[64] = {0};
    {
        SideWorker::Job j = w.submit([&owner] { nap(20); for (int i = 0; i < 64; ++i) owner[i] = i + 1; throw std::runtime_error("swallowed"); });
    }
    for (int i = 0; i < 64; ++i) CHECK(owner[i] == i + 1);
    CHECK(!w.pending());
    SideWorker::Job j = w.submit([] {});
    CHECK(what_of(j).empty());                           // the destroyed handle took its job's error with it
    {
        SideWorker::Job k = w.submit([&owner] { nap(5); owner[0] = -1; });
        k.reset();                                       // the destructor's join, by name
        CHECK(owner[0] == -1 && !k.pending());
    }
    std::printf("ok dtor\n");
}

static void case_order() {
    SideWorker w;
    std::mutex m;
    std::condition_variable cv;
    bool go = false;
    std::atomic<int> first_ended{0}, second_saw{-1};
    SideWorker::Job a = w.submit([&] { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return go; }); nap(5); first_ended = 1; });
    std::thread opener([&] { nap(20); { std::lock_guard<std::mutex> lk(m); go = true; } cv.notify_all(); });
    SideWorker::Job b = w.submit([&] { second_saw = first_ended.load(); });      // blocks in submit() until the first job ended
    CHECK(first_ended == 1);
    b.wait();
    CHECK(second_saw == 1);
    CHECK(a.pending());                                  // still owns its (finished) job: the join is immediate
    a.wait();
    opener.join();
    std::printf("ok order\n");
}

static void case_unjoined() {
    SideWorker w;
    int x = 0;
    SideWorker::Job j = w.submit([] { throw std::runtime_error("kept"); });
    j = w.submit([&x] { x = 3; });                       // nobody joined the first job: its error is not the old handle's to drop any more
    CHECK(what_of(j) == "kept" && x == 3);
    j = w.submit([] {});
    CHECK(what_of(j).empty());                           // handed out once
    std::printf("ok unjoined\n");
}

static void case_move() {
    SideWorker w;
    std::atomic<int> runs{0};
    SideWorker::Job a = w.submit([&] { nap(5); ++runs; throw std::runtime_error("moved"); });
    SideWorker::Job b = std::move(a);
    CHECK(!a.pending() && b.pending());
    a.wait(); a.reset();                                 // the source is empty: no second join, no error
    CHECK(what_of(b) == "moved" && runs == 1 && !b.pending());
    // move assignment joins the job it replaces (and swallows its error) before it takes the new one over
    int y = 0;
    SideWorker w2;
    SideWorker::Job c = w.submit([&y] { nap(10); y = 1; throw std::runtime_error("replaced"); });
    SideWorker::Job d = w2.submit([&y] { nap(1); });
    c = std::move(d);
    CHECK(y == 1 && c.pending() && !d.pending());
    CHECK(what_of(c).empty());
    SideWorker::Job e = w.submit([] {});
    CHECK(what_of(e).empty());
    std::printf("ok move\n");
}

static void case_rounds() {
    {
        SideWorker w;
        long sum = 0;
        for (int i = 1; i <= 1000; ++i) { SideWorker::Job j = w.submit([&sum, i] { sum += i; }); j.wait(); }
        CHECK(sum == 500500);
        nap(2);                                          // destroyed while its thread is parked
    }
    { SideWorker never_used; }
    { SideWorker w; int x = 0; { SideWorker::Job j = w.submit([&x] { x = 1; }); } CHECK(x == 1); }
    std::printf("ok rounds\n");
}

int main() {
    case_run(); case_throw(); case_dtor(); case_order(); case_unjoined(); case_move(); case_rounds();
    return 0;
}
"""

CASES = ["run", "throw", "dtor", "order", "unjoined", "move", "rounds"]
BUILDS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_side_worker_program(tmp_path, build):
    cpp = tmp_path / "side_worker_host.cpp"
    cpp.write_text(SRC)
    exe = tmp_path / f"side_worker_host_{build}"
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *BUILDS[build], "-I", CSRC, str(cpp), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [w for c in CASES for w in ("ok", c)], r.stdout
    assert r.stderr == "", r.stderr
