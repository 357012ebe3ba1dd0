// One wave's n_fft 2048 transform of afx_melfused2.hip restated lane by lane in float32, with the W_64 twiddles applied on either
// side of exchange 2: by the writer (15 products per lane against rows of W_64^(m2 j1), the form up to round 9) or by the reader
// (3 products per base against row q >> 4 of the round-10 table).  Built on the project's own pieces -- dft4 / dft16 / rev4
// (afx_pkmath.h), split_pair (afx_melparts.h) and the emulated cmul / fma of tests/emu/hip/afx_asm.h -- so a product has the
// bits the device gives it.  tests/test_mel_tw2_cpu.py compares the 1025 power bins of the two forms.  Test infrastructure.
#include "hip/hip_runtime.h"
namespace {
alignas(16) unsigned char smem[16];
}
static unsigned char *const afx_emu_lds = smem;  // (afx_melparts.h's band stage names them; nothing here reads the LDS)
static inline void afx_emu_ds() {}
#include "afx_melparts.h"

namespace {
const double PI = 3.14159265358979323846;
v2 tw(double num, double den, double scale = 1.0) {
    const double ang = -2.0 * PI * num / den;  // twiddles in double, rounded once: fill_tables' expression
    return v2{(float)(scale * cos(ang)), (float)(scale * sin(ang))};
}
}  // namespace

// the writer-side table of rounds 2-9, [4][16]: entry (m, j) = W_64^(m j) as (re, im)
extern "C" void afx_tw2_old_table(float *t) {
    for (int m = 0; m < 4; ++m)
        for (int j = 0; j < 16; ++j) {
            const v2 w = tw((double)(m * j), 64.0);
            t[2 * (16 * m + j)] = w.x;
            t[2 * (16 * m + j) + 1] = w.y;
        }
}

// x: 2048 samples, win: 2048 window values, power: 1025 bins |X|^2.  readerSide: where the W_64 twiddles are applied
extern "C" void afx_tw2_wave(const float *x, const float *win, int readerSide, float *power) {
    static v2 ex1[64][16], img[256][4];
    for (int lane = 0; lane < 64; ++lane) {  // window, radix-16 over n1, W_1024^(lane k1), exchange 1: Y[n2 = lane][k1]
        v2 v[16];
        for (int n1 = 0; n1 < 16; ++n1) {
            const int n = 64 * n1 + lane;
            v[n1] = v2{x[2 * n] * win[2 * n], x[2 * n + 1] * win[2 * n + 1]};
        }
        dft16(v);
        ex1[lane][0] = v[0];
        for (int k = 1; k < 16; ++k) ex1[lane][k] = cmul(v[rev4(k)], tw((double)(k * lane), 1024.0));
    }
    for (int lane = 0; lane < 64; ++lane) {  // radix-16 over m1 -> image V[q = k1 + 16 j1][m2]
        const int k1 = lane >> 2, m2 = lane & 3;
        v2 v[16];
        for (int m1 = 0; m1 < 16; ++m1) v[m1] = ex1[4 * m1 + m2][k1];
        dft16(v);
        for (int j1 = 0; j1 < 16; ++j1) {
            v2 o = v[rev4(j1)];
            if (!readerSide && j1 > 0) o = cmul(o, tw((double)(m2 * j1), 64.0));  // (m2 = 0 included: (1, -0), as the kernel had it)
            img[k1 + 16 * j1][m2] = o;
        }
    }
    for (int lane = 0; lane < 64; ++lane) {  // last radix-4 + real-input split, 513 pairs on 512 slots
        const bool lane0 = lane == 0;
        for (int s = 0; s < 2; ++s) {
            const int qa = lane + 64 * s, qb = s == 0 ? (lane0 ? 128 : 256 - lane) : 192 - lane;
            v2 za[4], zb[4];
            for (int m = 0; m < 4; ++m) {
                za[m] = img[qa][m];
                zb[m] = img[qb][m];
                if (readerSide && m > 0) {  // (row 0 included: (1, -0))
                    za[m] = cmul(za[m], tw((double)(m * (qa >> 4)), 64.0));
                    zb[m] = cmul(zb[m], tw((double)(m * (qb >> 4)), 64.0));
                }
            }
            dft4(za[0], za[1], za[2], za[3]);
            dft4(zb[0], zb[1], zb[2], zb[3]);
            v2 A[4] = {za[0], za[1], za[2], za[3]}, B[4] = {zb[3], zb[2], zb[1], zb[0]};
            int bin[4] = {qa, qa + 256, qa + 512, qa + 768};
            if (s == 0) {
                if (lane0) power[512] = za[2].x * za[2].x + za[2].y * za[2].y;
                if (lane0) {
                    A[2] = zb[0], A[3] = zb[1];
                    B[0] = za[0], B[1] = za[3], B[2] = zb[3], B[3] = zb[2];
                    bin[2] = 128, bin[3] = 384;
                }
            }
            for (int j = 0; j < 4; ++j) split_pair(A[j], B[j], tw((double)bin[j], 2048.0, 0.5), power[bin[j]], power[1024 - bin[j]]);
        }
    }
}
