"""csrc/fdjac_dispatch.h on its own (no GPU, no HIP): fd_pick, the picker every kernel launcher goes through from a runtime value to
a template argument, compiled with g++ and exercised by a small program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "fdjac_dispatch.h"
#include <cstdio>

constexpr int kRegColors = 8;
template <int V> struct Tag { static constexpr int value = V; };
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    // a matching value: the callable runs exactly once, with that constant (usable as a template argument)
    int calls = 0, got = -1;
    CHECK((fd_pick<0, 1, 2>(1, [&](auto M) { ++calls; got = Tag<M()>::value; })));
    CHECK(calls == 1 && got == 1);
    // no match: nothing runs, false
    calls = 0;
    CHECK((!fd_pick<0, 1, 2>(3, [&](auto) { ++calls; })));
    CHECK((!fd_pick<0, 1, 2>(-1, [&](auto) { ++calls; })));
    CHECK(calls == 0);
    // nested pickers: every combination exactly once over all inputs, and nothing else
    int hit2[2][2] = {}, hit3[3][3] = {};
    for (int m = 0; m < 2; ++m)
        for (int nl = 0; nl < 2; ++nl)
            CHECK((fd_pick<0, 1>(m, [&](auto M) { fd_pick<false, true>(nl != 0, [&](auto NL) { ++hit2[Tag<M()>::value][NL() ? 1 : 0]; }); })));
    for (int m = 0; m < 2; ++m)
        for (int nl = 0; nl < 2; ++nl) CHECK(hit2[m][nl] == 1);
    for (int m = 0; m < 3; ++m)
        for (int sk = 0; sk < 3; ++sk)
            CHECK((fd_pick<0, 1, 2>(m, [&](auto M) { fd_pick<0, 1, 2>(sk, [&](auto SK) { ++hit3[M()][Tag<SK()>::value]; }); })));
    for (int m = 0; m < 3; ++m)
        for (int sk = 0; sk < 3; ++sk) CHECK(hit3[m][sk] == 1);
    // mixed int / bool candidates, either kind of runtime value
    int mixed = 0;
    CHECK((fd_pick<false, 1, 2>(2, [&](auto V) { mixed += (int)V(); })));
    CHECK((fd_pick<0, true>(true, [&](auto V) { mixed += 10 * (int)V(); })));
    CHECK((fd_pick<0, true>(false, [&](auto V) { mixed += 100 + (int)V(); })));
    CHECK(mixed == 112);
    // bucket, then pick: a range choice whose last arm is a default
    const int in[6] = {1, 4, 5, 6, 7, kRegColors}, want[6] = {4, 4, 6, 6, 8, 8};
    for (int i = 0; i < 6; ++i) {
        const int C = in[i], ncc = C <= 4 ? 4 : C <= 6 ? 6 : kRegColors;
        int nc = 0, n = 0;
        CHECK((fd_pick<4, 6, kRegColors>(ncc, [&](auto NC) { nc = Tag<NC()>::value; ++n; })));
        CHECK(n == 1 && nc == want[i]);
    }
    return 0;
}
"""


def test_fd_pick_calls_the_matching_candidate_once_and_nothing_otherwise(tmp_path):
    src = tmp_path / "pick.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "pick")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "finitediff.jl_amd", "csrc"),
                           str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
