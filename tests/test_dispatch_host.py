"""CPU: csrc/dsce_dispatch.h (the launchers' run-time value -> template argument
helpers) in a stand-alone C++17 program: which values reach f, with which
constant, and what the helpers return."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "channel-estimation_amd", "csrc")

PROGRAM = r"""
#include "dsce_dispatch.h"
#include <cstdio>
using namespace dsce;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

template <int A, int B> struct Pair { static int code() { return 100 * A + B; } };

// for_value<Vs...> / for_range<Lo, Hi> over Lo - 2 .. Hi + 2: a listed value gives
// one call with the constant equal to it and true, any other no call and false
template <class Dispatch>
static void sweep(int lo, int hi, bool (*listed)(int), Dispatch d) {
    for (int v = lo - 2; v <= hi + 2; ++v) {
        int calls = 0, got = -1000;
        const bool hit = d(v, [&](auto C) {
            static_assert(decltype(C)::value == C, "the constant converts to its value");
            ++calls;
            got = C;
        });
        if (listed(v)) CHECK(hit && calls == 1 && got == v);
        else CHECK(!hit && calls == 0);
    }
}

int main() {
    sweep(1, 8, [](int v) { return v == 1 || v == 2 || v == 4 || v == 8; },
          [](int v, auto f) { return for_value<1, 2, 4, 8>(v, f); });
    sweep(-3, 28, [](int v) { return v == -3 || v == 16 || v == 24 || v == 28; },
          [](int v, auto f) { return for_value<16, 28, -3, 24>(v, f); });
    sweep(5, 5, [](int v) { return v == 5; }, [](int v, auto f) { return for_value<5>(v, f); });
    sweep(9, 20, [](int v) { return v >= 9 && v <= 20; }, [](int v, auto f) { return for_range<9, 20>(v, f); });
    sweep(-1, 1, [](int v) { return v >= -1 && v <= 1; }, [](int v, auto f) { return for_range<-1, 1>(v, f); });
    sweep(7, 7, [](int v) { return v == 7; }, [](int v, auto f) { return for_range<7, 7>(v, f); });

    // for_bool: both arms, one call each, the constant usable as a template argument
    for (int b = 0; b < 2; ++b) {
        int calls = 0, got = -1;
        for_bool(b != 0, [&](auto B) {
            ++calls;
            got = Pair<B, 7>::code();
        });
        CHECK(calls == 1 && got == 100 * b + 7);
    }

    // nested: the pair reaches the template, and an inner miss is visible to the caller
    for (int a = 15; a <= 25; ++a)
        for (int b = 3; b <= 9; ++b) {
            bool hit = false;
            int calls = 0, got = -1;
            const bool outer = for_value<16, 24>(a, [&](auto A) {
                hit = for_range<4, 8>(b, [&](auto B) {
                    ++calls;
                    got = Pair<A, B>::code();
                });
            });
            const bool in_a = a == 16 || a == 24, in_b = b >= 4 && b <= 8;
            CHECK(outer == in_a);
            CHECK(hit == (in_a && in_b));
            CHECK(calls == (in_a && in_b ? 1 : 0));
            if (in_a && in_b) CHECK(got == 100 * a + b);
        }
    if (!fails) std::printf("ok\n");
    return fails ? 1 : 0;
}
"""


def test_dispatch_helpers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not (os.path.isabs(cxx) and os.access(cxx, os.X_OK)):
        pytest.skip("no C++ compiler (g++ or ROCm's clang++)")
    src, exe = tmp_path / "dispatch_host.cpp", tmp_path / "dispatch_host"
    src.write_text(PROGRAM)
    cc = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
