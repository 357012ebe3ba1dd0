"""CPU: the plain-C twins of afx_frameops.h -- what the emulated builds compile in place of the hand-issued sequences.

A small host program includes the header the way the emulated builds do (the lane emulator's hip_runtime.h first, so the twins
are chosen) and checks, bit for bit:
  * pair_power(e2, wo) against |x|^2 = x.x * x.x + x.y * x.y and |y|^2 of x = e2 / 2 + wo, y = e2 / 2 - wo formed the way split_pair
    formed them before round 8 (one fma per component, then two products and a sum with separate roundings: the program is
    compiled with contraction off), on random values, denormals, zeros, huge values and values whose squares overflow;
  * shift_rows_inplace + rows_fetch_new_s against the image moved down by S rows and refilled from base + lane offset + 512 k bytes;
  * max4_floor / max_floor against fmaxf(x, 1e-8f), a quiet NaN included (1e-8 from both)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang"
INC = [f"-I{EMU}", f"-I{EMU}/hip", f"-I{ROOT}/include", f"-I{ROOT}/audioflux_amd/csrc/hip", f"-I{ROOT}/audioflux_amd/csrc/host"]

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs clang (ext_vector_type)")

PROGRAM = r"""
#include <hip/hip_runtime.h>
#include <afx_frameops.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#ifndef AFX_EMU_HIP_RUNTIME_H
#error "the lane emulator's hip_runtime.h must come first on the include path"
#endif

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

// split_pair's power before round 8: x = e2 * 0.5f + wo and y = e2 * 0.5f - wo as one fma per component, then
// fl(fl(x.x^2) + fl(x.y^2)) (this file is compiled with -ffp-contract=off)
static void old_form(const float e2[2], const float wo[2], float &pk, float &pq) {
    const float xx = fmaf(e2[0], 0.5f, wo[0]), xy = fmaf(e2[1], 0.5f, wo[1]);
    const float yx = fmaf(e2[0], 0.5f, -wo[0]), yy = fmaf(e2[1], 0.5f, -wo[1]);
    const float a = xx * xx, b = xy * xy, c = yx * yx, d = yy * yy;
    pk = a + b;
    pq = c + d;
}

int main() {
    std::mt19937 rng(8);
    std::uniform_real_distribution<float> uni(-1.f, 1.f);
    const float special[] = {0.f, -0.f, 1e-45f, -1e-45f, 1.1754942e-38f, 1e-38f, 1e-30f, 1e-20f, 3e-8f, 1.f, -1.f, 3.f, 1e10f, -1e19f, 1.8e19f, 2e19f,
                             3.3e38f, -3.4028235e38f};
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    std::vector<float> pool(special, special + ns);
    for (int i = 0; i < 64; ++i) pool.push_back(uni(rng) * std::ldexp(1.f, (int)(rng() % 80) - 40));
    long n = 0, bad = 0;
    auto check = [&](float a, float b, float c, float d) {
        const float e2[2] = {a, b}, wo[2] = {c, d};
        float pk, pq;
        old_form(e2, wo, pk, pq);
        const v2 p = pair_power(v2{a, b}, v2{c, d});
        ++n;
        if (!same(p.x, pk) || !same(p.y, pq)) {
            if (bad++ < 5) printf("pair_power(%a, %a; %a, %a) = %a, %a, want %a, %a\n", a, b, c, d, p.x, p.y, pk, pq);
        }
    };
    for (float a : pool)
        for (float b : special)
            for (float c : pool)
                for (float d : special) check(a, b, c, d);
    for (int i = 0; i < 200000; ++i) {
        const float s = std::ldexp(1.f, (int)(rng() % 60) - 30);
        check(uni(rng) * s, uni(rng) * s, uni(rng) * s, uni(rng) * s);
    }
    printf("pair_power: %ld cases, %ld differ\n", n, bad);

    // the image of overlapping frames: rows 512 bytes apart, lane offset in bytes
    long badRows = 0;
    std::vector<float> mem(16 * 128 + 64);
    for (size_t i = 0; i < mem.size(); ++i) mem[i] = (float)i;
    auto rows = [&](auto tag) {
        constexpr int S = decltype(tag)::value;
        for (unsigned lane = 0; lane < 64; lane += 21) {
            v2 r[16], want[16];
            for (int k = 0; k < 16; ++k) r[k] = want[k] = v2{(float)(1000 + k), (float)(-1000 - k)};
            for (int k = 0; k + S < 16; ++k) want[k] = want[k + S];
            for (int k = 0; k < S; ++k) want[16 - S + k] = v2{mem[16 + 128 * k + 2 * lane], mem[16 + 128 * k + 2 * lane + 1]};
            shift_rows_inplace<S>(r);
            rows_fetch_new_s<S, false>(r, 8u * lane, mem.data() + 16);
            for (int k = 0; k < 16; ++k) badRows += !(same(r[k].x, want[k].x) && same(r[k].y, want[k].y));
        }
    };
    rows(std::integral_constant<int, 2>());
    rows(std::integral_constant<int, 4>());
    rows(std::integral_constant<int, 8>());
    printf("rows_fetch_new_s: %ld values differ\n", badRows);

    long badMax = 0;
    const float mx[] = {0.f, -0.f, 1e-45f, 9.9e-9f, 1e-8f, 1.0000001e-8f, 1.f, -1.f, 3.3e38f, INFINITY, -INFINITY, NAN};
    for (float x : mx) {
        const float want = fmaxf(x, 1e-8f);
        const fo_v4 q = max4_floor(fo_v4{x, x, x, x});
        badMax += !(same(max_floor(x), want) && same(q.x, want) && same(q.y, want) && same(q.z, want) && same(q.w, want));
    }
    badMax += !(max_floor(NAN) == 1e-8f);
    printf("max_floor: %ld values differ\n", badMax);
    if (bad || badRows || badMax) return 1;
    printf("OK\n");
    return 0;
}
"""


def test_frameops_twins_bit_equal_to_the_plain_forms(tmp_path):
    src, exe = tmp_path / "frameops_twins.cpp", tmp_path / "frameops_twins"
    src.write_text(PROGRAM)
    r = subprocess.run([CLANG + "++", "-std=c++17", "-O2", "-ffp-contract=off", *INC, str(src), "-o", str(exe), "-lm", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout


def test_twins_keep_their_roundings_with_contraction_on(tmp_path):
    """the emulated builds do not pass -ffp-contract=off: the twin carries its own pragma, so the same program must pass when
    only the twin's translation unit allows contraction (the reference form is then written with explicit roundings)"""
    prog = PROGRAM.replace("const float a = xx * xx, b = xy * xy, c = yx * yx, d = yy * yy;",
                           "volatile float a = xx * xx, b = xy * xy, c = yx * yx, d = yy * yy;")
    src, exe = tmp_path / "frameops_twins_fast.cpp", tmp_path / "frameops_twins_fast"
    src.write_text(prog)
    r = subprocess.run([CLANG + "++", "-std=c++17", "-O2", "-ffp-contract=fast", *INC, str(src), "-o", str(exe), "-lm", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout
