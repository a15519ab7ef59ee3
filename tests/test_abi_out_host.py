"""Host check of csrc/abi_out.hpp, the owner of the result handles of a C ABI entry point, compiled with g++ into a stand-alone program (no GPU,
no HIP).  The handle type of the program counts its live instances.  The program checks, each as a numbered case that prints "ok <name>":

  commit     one handle, a group of three and a per-member array reach their slots at commit(), not before; the owner holds nothing afterwards
  abandon    an owner destroyed without commit() after 0, some and all handles were made: every slot is unchanged, no handle is left alive
  throw      an exception between two additions (the solver threw part-way): the slots keep their sentinel, the first handle is deleted
  skipped    a batched array nulled up front in which some members are skipped: their slots stay null, with and without commit()
  twice      commit() twice is harmless: the second writes nothing, the owner's destructor deletes nothing the caller owns

The program is built and run three times: plain, with -fsanitize=address,undefined -fno-sanitize-recover=all, and with -Werror -Wall -Wextra;
every run must exit 0 with all cases reported and nothing on stderr."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")

SRC = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include "abi_out.hpp"

struct Handle {
    static int live;
    int payload = 0;
    Handle() { ++live; }
    ~Handle() { --live; }
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
};
int Handle::live = 0;
using Out = dre::AbiOut<Handle>;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static Handle* const SENTINEL = reinterpret_cast<Handle*>(static_cast<std::uintptr_t>(0x5e5e5e50));

static void case_commit() {
    {   // one handle
        Handle* x = SENTINEL;
        Out o;
        Handle* h = o.make(&x);
        h->payload = 7;
        CHECK(x == SENTINEL && Handle::live == 1);
        o.commit();
        CHECK(x == h && x->payload == 7 && Handle::live == 1);
        delete x;
    }
    {   // a group: U, S, V
        Handle *u = SENTINEL, *s = SENTINEL, *v = SENTINEL;
        {
            Out o;
            Handle* hu = o.make(&u); Handle* hs = o.make(&s); Handle* hv = o.make(&v);
            CHECK(u == SENTINEL && s == SENTINEL && v == SENTINEL && Handle::live == 3);
            o.commit();
            CHECK(u == hu && s == hs && v == hv);
        }
        CHECK(Handle::live == 3);          // the owner's destructor left the committed handles alone
        delete u; delete s; delete v;
    }
    {   // a per-member array
        Handle* arr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        {
            Out o;
            for (int b = 0; b < 5; ++b) o.make(arr + b)->payload = 10 + b;
            for (int b = 0; b < 5; ++b) CHECK(arr[b] == nullptr);
            o.commit();
        }
        for (int b = 0; b < 5; ++b) { CHECK(arr[b] && arr[b]->payload == 10 + b); delete arr[b]; }
    }
    CHECK(Handle::live == 0);
    std::printf("ok commit\n");
}

static void case_abandon() {
    for (int made = 0; made <= 3; ++made) {          // 0, some (1, 2) and all (3) of a group of three
        Handle* slot[3] = {SENTINEL, SENTINEL, SENTINEL};
        {
            Out o;
            for (int i = 0; i < made; ++i) o.make(slot + i);
            CHECK(Handle::live == made);
        }
        CHECK(Handle::live == 0);
        for (int i = 0; i < 3; ++i) CHECK(slot[i] == SENTINEL);
    }
    std::printf("ok abandon\n");
}

static void case_throw() {
    Handle *x = SENTINEL, *y = SENTINEL;
    bool caught = false;
    try {
        Out o;
        o.make(&x);
        if (Handle::live == 1) throw std::runtime_error("solver failed");
        o.make(&y);
        o.commit();
    } catch (const std::runtime_error&) { caught = true; }
    CHECK(caught && x == SENTINEL && y == SENTINEL && Handle::live == 0);
    std::printf("ok throw\n");
}

static void case_skipped() {
    for (int commit = 0; commit <= 1; ++commit) {
        Handle* arr[4];
        for (Handle*& p : arr) p = nullptr;          // the batched calls null their arrays up front
        {
            Out o;
            for (int b = 0; b < 4; ++b) if (b != 1 && b != 3) o.make(arr + b);          // members 1 and 3 failed
            if (commit) o.commit();
        }
        CHECK(arr[1] == nullptr && arr[3] == nullptr);
        if (commit) { CHECK(arr[0] && arr[2] && Handle::live == 2); delete arr[0]; delete arr[2]; }
        else CHECK(arr[0] == nullptr && arr[2] == nullptr);
        CHECK(Handle::live == 0);
    }
    std::printf("ok skipped\n");
}

static void case_twice() {
    Handle *x = SENTINEL, *y = SENTINEL;
    {
        Out o;
        Handle* h = o.make(&x);
        o.commit();
        CHECK(x == h);
        x = SENTINEL;                       // (a second commit that wrote again would put h back)
        o.commit();
        CHECK(x == SENTINEL && Handle::live == 1);
        Handle* g = o.make(&y);             // the owner goes on working after a commit
        o.commit(); o.commit();
        CHECK(y == g && x == SENTINEL && Handle::live == 2);
        delete h;
    }
    CHECK(Handle::live == 1);
    delete y;
    CHECK(Handle::live == 0);
    std::printf("ok twice\n");
}

int main() {
    case_commit(); case_abandon(); case_throw(); case_skipped(); case_twice();
    return 0;
}
"""

CASES = ["commit", "abandon", "throw", "skipped", "twice"]
BUILDS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "strict": ["-Werror", "-Wall", "-Wextra"]}


@pytest.mark.parametrize("build", list(BUILDS))
def test_abi_out_program(tmp_path, build):
    cpp = tmp_path / "abi_out_host.cpp"
    cpp.write_text(SRC)
    exe = tmp_path / f"abi_out_host_{build}"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *BUILDS[build], "-I", CSRC, str(cpp), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == [w for c in CASES for w in ("ok", c)], r.stdout
    assert r.stderr == "", r.stderr


def test_abi_out_header_is_hip_free():
    """The header includes neither common.hpp nor HIP: that is what lets the program above be plain g++."""
    txt = open(os.path.join(CSRC, "abi_out.hpp")).read()
    includes = [ln.split()[1] for ln in txt.splitlines() if ln.startswith("#include")]
    assert includes and all(inc.startswith("<") and "hip" not in inc for inc in includes), includes
