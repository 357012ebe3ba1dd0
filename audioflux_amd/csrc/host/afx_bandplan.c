/* afx_bandplan.c -- turns a filter-bank matrix into the per-lane banded view
 * the fused kernel consumes (AfxBandPlan, afx_device.h).
 *
 * Triangular / window-shaped auditory banks are banded: each row's non-zeros
 * sit in one short contiguous bin range (mel-128 @ n_fft 2048: 2025 non-zeros
 * of 131 200, <= 2 per column).  The reference multiplies the full dense
 * matrix (src/vector/flux_vector.c:55-86); zero weights contribute exact
 * zeros, so summing only the band in ascending bin order gives the same value.
 * Rows are sorted by band length and dealt to the 64 lanes: lane i gets the
 * i-th longest row as "A" and, when num > 64, one of the short rows as "B"
 * (longest A with shortest B) to even the work out.
 *
 * Three plans are made here: whole rows in an A and a B slot per lane (afx_bandplan_build), row segments for banks whose
 * rows are longer than the compiled tap variants (afx_bandplan_build_split), and the packed form of a whole-row plan
 * (afx_bandpack_build, at the end of the file): one stream of three partitions per lane that holds one, two or three rows
 * without the A / B padding -- 48 tap slots per lane instead of 64 at mel-128 / n_fft 2048.
 */
#include <stdlib.h>
#include <string.h>

#include "afx_device.h"
#include "afx_host.h"

typedef struct {
    int row, start, len;
} RowBand;

static int cmp_len_desc(const void *a, const void *b) {
    const RowBand *x = (const RowBand *)a, *y = (const RowBand *)b;
    if (x->len != y->len) return y->len - x->len;
    return x->row - y->row;
}

void afx_bandplan_free(AfxBandPlan *p) {
    if (!p) return;
    free(p->wA);
    free(p->wB);
    p->wA = p->wB = NULL;
}

/* ---- LDS-bank-aware lane assignment ------------------------------------------
 * In the kernel every lane reads the pairs P[start_lane + 2t .. +1], t = 0,1,2,...
 * with one ds_read_b64 per pair (start_lane even); ds_read_b64 sees 64 dword
 * banks, so a 32-lane half-wave is conflict-free exactly when its 32 values of
 * start/2 are distinct mod 32.  A row may start up to `d` bins early (leading
 * zero weights) to land on a free residue.  Rows are matched to the 64 (half, residue) slots so that the
 * longest padded row, max(len + d), is as short as possible: bottleneck
 * assignment by binary search over the bound + Kuhn's augmenting-path matching
 * (64 x 64, plan time only). */
static int shift_for(const RowBand *r, int residue) {
    int d = (r->start - 2 * residue) % 64;
    if (d < 0) d += 64;
    return d; /* new start = start - d is even and (start - d)/2 is congruent to residue mod 32 */
}

static int try_augment(int row, int n, const RowBand *rows, int bound, int *slotOwner, char *seen) {
    (void)n;
    for (int slot = 0; slot < 64; slot++) {
        if (seen[slot]) continue;
        const int d = shift_for(&rows[row], slot & 31);
        if (d > rows[row].start || rows[row].len + d > bound) continue;
        seen[slot] = 1;
        if (slotOwner[slot] < 0 ||
            try_augment(slotOwner[slot], n, rows, bound, slotOwner, seen)) {
            slotOwner[slot] = row;
            return 1;
        }
    }
    return 0;
}

static int match_with_bound(const RowBand *rows, int n, int bound, int *slotOwner) {
    for (int s = 0; s < 64; s++) slotOwner[s] = -1;
    for (int i = 0; i < n; i++) {
        char seen[64];
        memset(seen, 0, sizeof(seen));
        if (!try_augment(i, n, rows, bound, slotOwner, seen)) return 0;
    }
    return 1;
}

/* assigns n (<= 64) rows to lanes; returns the padded tap count, fills
 * laneRow[64] (index into rows, -1 = idle lane) and laneShift[64] */
static int assign_lanes(const RowBand *rows, int n, int *laneRow, int *laneShift) {
    int slotOwner[64];
    int lo = 1, hi = 1;
    for (int i = 0; i < n; i++) {
        if (rows[i].len > lo) lo = rows[i].len;
    }
    hi = lo + 63;
    if (!match_with_bound(rows, n, hi, slotOwner)) {
        /* cannot happen (a shift of < 32 always exists unless start is tiny and
         * residues clash); fall back to identity placement, conflicts allowed */
        for (int l = 0; l < 64; l++) {
            laneRow[l] = l < n ? l : -1;
            laneShift[l] = 0;
        }
        return lo;
    }
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (match_with_bound(rows, n, mid, slotOwner)) hi = mid; else lo = mid + 1;
    }
    match_with_bound(rows, n, lo, slotOwner);
    for (int slot = 0; slot < 64; slot++) { /* slot = 32*half + residue = lane */
        laneRow[slot] = slotOwner[slot];
        laneShift[slot] = slotOwner[slot] >= 0 ? shift_for(&rows[slotOwner[slot]], slot & 31) : 0;
    }
    return lo;
}

/* returns 0 and fills *p when the bank fits the banded scheme, 1 otherwise */
int afx_bandplan_build(const float *bank, int num, int F, AfxBandPlan *p) {
    memset(p, 0, sizeof(*p));
    if (!bank || num < 1 || num > 128) return 1;
    RowBand *rb = (RowBand *)calloc((size_t)num, sizeof(RowBand));
    if (!rb) return 1;
    for (int m = 0; m < num; m++) {
        const float *row = bank + (size_t)m * F;
        int first = -1, last = -1;
        for (int k = 0; k < F; k++) {
            if (row[k] != 0.f) {
                if (first < 0) first = k;
                last = k;
            }
        }
        rb[m].row = m;
        rb[m].start = first < 0 ? 0 : first;
        rb[m].len = first < 0 ? 0 : last - first + 1;
    }
    qsort(rb, (size_t)num, sizeof(RowBand), cmp_len_desc);

    /* the 64 longest rows form set A, the rest set B: every lane gets one of each */
    const int nA = num < 64 ? num : 64;
    const int nB = num - nA;
    int laneRowA[64], laneShiftA[64], laneRowB[64], laneShiftB[64];
    p->num = num;
    p->tapsA = assign_lanes(rb, nA, laneRowA, laneShiftA);
    p->tapsB = 1;
    for (int l = 0; l < 64; l++) {
        laneRowB[l] = -1;
        laneShiftB[l] = 0;
    }
    if (nB > 0) p->tapsB = assign_lanes(rb + nA, nB, laneRowB, laneShiftB);
    p->wA = (float *)calloc((size_t)p->tapsA * 64, sizeof(float));
    p->wB = (float *)calloc((size_t)p->tapsB * 64, sizeof(float));
    if (!p->wA || !p->wB) {
        free(rb);
        afx_bandplan_free(p);
        return 1;
    }
    for (int l = 0; l < 64; l++) {
        p->rowA[l] = p->rowB[l] = -1;
        /* idle lanes still execute the reads: give them their own residue so they
         * do not collide with a working lane of the same half */
        p->startA[l] = 2 * (l & 31);
        p->startB[l] = 2 * (l & 31);
        if (laneRowA[l] >= 0) {
            const RowBand *r = &rb[laneRowA[l]];
            const int d = laneShiftA[l];
            for (int t = 0; t < r->len; t++)
                p->wA[(size_t)(t + d) * 64 + l] = bank[(size_t)r->row * F + r->start + t];
            p->startA[l] = r->start - d;
            p->rowA[l] = r->row;
        }
        if (laneRowB[l] >= 0) {
            const RowBand *r = &rb[nA + laneRowB[l]];
            const int d = laneShiftB[l];
            for (int t = 0; t < r->len; t++)
                p->wB[(size_t)(t + d) * 64 + l] = bank[(size_t)r->row * F + r->start + t];
            p->startB[l] = r->start - d;
            p->rowB[l] = r->row;
        }
    }
    free(rb);
    return 0;
}

/* ---- split plans ---------------------------------------------------------------------------
 * Banks whose rows are longer than the compiled tap variants (mel-40 / mel-64, bark and erb banks,
 * higher sample rates) still have ~2 non-zeros per bin in total: their rows are cut into
 * segments of at most tapsA (A slots) or tapsB (B slots) bins, every lane gets one A and one B
 * segment, and the kernel adds a row's segment results in ascending bin order.  Segment starts are
 * matched to LDS-bank residues like whole rows; because a segment may have to start a few bins
 * early, the payload per slot is reduced until the padded segments fit the variant.
 * rowCap = floats of the kernel's zero-padded power row: no slot may read beyond it.
 * Returns 0 and fills *p (split = 1) when the bank fits, 1 otherwise. */
int afx_bandplan_build_split(const float *bank, int num, int F, int tapsA, int tapsB, int rowCap,
                             AfxBandPlan *p) {
    memset(p, 0, sizeof(*p));
    if (!bank || num < 1 || num > 128 || tapsA < 4 || tapsB < 4) return 1;
    RowBand *rb = (RowBand *)calloc((size_t)num, sizeof(RowBand));
    RowBand *segA = (RowBand *)calloc(64, sizeof(RowBand)), *segB = (RowBand *)calloc(64, sizeof(RowBand));
    if (!rb || !segA || !segB) {
        free(rb);
        free(segA);
        free(segB);
        return 1;
    }
    for (int m = 0; m < num; m++) {
        const float *row = bank + (size_t)m * F;
        int first = -1, last = -1;
        for (int k = 0; k < F; k++)
            if (row[k] != 0.f) {
                if (first < 0) first = k;
                last = k;
            }
        rb[m].row = m;
        rb[m].start = first < 0 ? 0 : first;
        rb[m].len = first < 0 ? 0 : last - first + 1;
    }
    int laneA[64], shiftA[64], laneB[64], shiftB[64];
    /* segment lists per row: type (0 A, 1 B) and index into segA / segB, ascending bins */
    unsigned char segType[128][4], segOf[128][4], segCnt[128];
    int payA = tapsA, payB = tapsB, ok = 0, nA = 0, nB = 0;
    for (int iter = 0; iter < 40 && !ok && payA >= 8 && payB >= 0; iter++) {
        nA = nB = 0;
        int feasible = 1;
        for (int m = 0; m < num && feasible; m++) {
            int rem = rb[m].len, pos = rb[m].start;
            segCnt[m] = 0;
            while (rem > 0) {
                if (segCnt[m] == 4) {
                    feasible = 0;
                    break;
                }
                const int c = segCnt[m]++;
                if (rem <= payB && nB < 64) {
                    segB[nB].row = m, segB[nB].start = pos, segB[nB].len = rem;
                    segType[m][c] = 1, segOf[m][c] = (unsigned char)nB++;
                    rem = 0;
                } else {
                    if (nA == 64) {
                        feasible = 0;
                        break;
                    }
                    const int take = rem < payA ? rem : payA;
                    segA[nA].row = m, segA[nA].start = pos, segA[nA].len = take;
                    segType[m][c] = 0, segOf[m][c] = (unsigned char)nA++;
                    pos += take, rem -= take;
                }
            }
        }
        if (!feasible) break; /* smaller payloads only make more segments */
        int needA = nA ? assign_lanes(segA, nA, laneA, shiftA) : 1;
        int needB = nB ? assign_lanes(segB, nB, laneB, shiftB) : 1;
        /* the kernel reads the power row in pairs: a placement that left a start odd (the
         * matcher's identity fallback) does not qualify */
        for (int l = 0; l < 64; l++) {
            if (nA && laneA[l] >= 0 && ((segA[laneA[l]].start - shiftA[l]) & 1)) needA = tapsA + 1;
            if (nB && laneB[l] >= 0 && ((segB[laneB[l]].start - shiftB[l]) & 1)) needB = tapsB + 1;
            /* a short segment near the top of the spectrum must not read past the row's zero pad:
             * start it 64 bins (one full residue cycle) earlier while its taps allow */
            if (nA && laneA[l] >= 0) {
                const RowBand *g = &segA[laneA[l]];
                while (g->start - shiftA[l] + tapsA > rowCap && shiftA[l] + 64 + g->len <= tapsA &&
                       g->start - shiftA[l] - 64 >= 0)
                    shiftA[l] += 64;
                if (g->start - shiftA[l] + tapsA > rowCap) needA = tapsA + 1;
            }
            if (nB && laneB[l] >= 0) {
                const RowBand *g = &segB[laneB[l]];
                while (g->start - shiftB[l] + tapsB > rowCap && shiftB[l] + 64 + g->len <= tapsB &&
                       g->start - shiftB[l] - 64 >= 0)
                    shiftB[l] += 64;
                if (g->start - shiftB[l] + tapsB > rowCap) needB = tapsB + 1;
            }
        }
        if (needA <= tapsA && needB <= tapsB) ok = 1;
        else {
            if (needA > tapsA) payA -= 2;
            if (needB > tapsB) payB -= 2;
        }
    }
    if (ok) {
        p->num = num;
        p->split = 1;
        p->tapsA = tapsA;
        p->tapsB = tapsB;
        p->wA = (float *)calloc((size_t)tapsA * 64, sizeof(float));
        p->wB = (float *)calloc((size_t)tapsB * 64, sizeof(float));
        if (!p->wA || !p->wB) {
            afx_bandplan_free(p);
            ok = 0;
        }
    }
    if (ok) {
        int slotOfA[64], slotOfB[64]; /* segment index -> lane */
        for (int l = 0; l < 64; l++) {
            p->rowA[l] = p->rowB[l] = -1;
            p->startA[l] = 2 * (l & 31);
            p->startB[l] = 2 * (l & 31);
            if (nA && laneA[l] >= 0) {
                const RowBand *g = &segA[laneA[l]];
                for (int t = 0; t < g->len; t++)
                    p->wA[(size_t)(t + shiftA[l]) * 64 + l] = bank[(size_t)g->row * F + g->start + t];
                p->startA[l] = g->start - shiftA[l];
                slotOfA[laneA[l]] = l;
            }
            if (nB && laneB[l] >= 0) {
                const RowBand *g = &segB[laneB[l]];
                for (int t = 0; t < g->len; t++)
                    p->wB[(size_t)(t + shiftB[l]) * 64 + l] = bank[(size_t)g->row * F + g->start + t];
                p->startB[l] = g->start - shiftB[l];
                slotOfB[laneB[l]] = l;
            }
        }
        for (int m = 0; m < 128; m++) {
            unsigned packed = 0;
            for (int c = 0; c < 4; c++) {
                unsigned slot = 128;
                if (m < num && c < segCnt[m])
                    slot = segType[m][c] ? 64u + (unsigned)slotOfB[segOf[m][c]] : (unsigned)slotOfA[segOf[m][c]];
                packed |= slot << (8 * c);
            }
            p->segIdx[m] = packed;
        }
    }
    free(rb);
    free(segA);
    free(segB);
    return ok ? 0 : 1;
}

/* ---- packed plans --------------------------------------------------------------------------
 * A whole-row plan pads its 64 longest rows to tapsA and its 64 shortest to tapsB: at mel-128 / n_fft 2048 the
 * (48, 16) variant runs 64 slots per lane for 31.6 real taps.  The packed plan (AfxBandPack, afx_bandpack.h) gives every
 * lane ONE stream of three partitions a | b | c in which a partition either continues the row before it or starts a
 * new one, so a lane holds one long row (a+b+c), two middling ones (a+b | c, a | b+c) or three short ones (a | b | c);
 * no lane can run fewer slots than the longest row has taps.  A row that occupies consecutive partitions is a CHAIN:
 * it has one power-row base, at an even bin (leading zero weights when its first bin is odd) and possibly a few bins
 * early to reach a free LDS bank pair, like shift_for above; the base of a continued partition is the chain's base plus
 * the taps before it.
 *
 * Planner: layouts are tried from the fewest slots; for a layout, x lanes carry one row, x carry three, y are (a+b | c)
 * and z are (a | b+c) with 2x + y + z = 64.  The rows, longest first, are dealt to the chains, roomiest first; every
 * (x, y, z) whose chains hold the rows that way is a candidate, ranked by the bank pairs its rows can reach.  Lanes are
 * then filled partition by partition: the chains that start at partition p are matched (Kuhn) to the (half, bank pair)
 * slots that the chains continuing into p leave free.  A chain left unmatched takes a free lane at its natural base
 * and its reads meet another lane's: the plan counts such lane pairs.  The matching is repeated over the candidates with
 * shuffled ties until a plan has no such pair, or the tries are used up and the plan with the fewest stays. */
#include "afx_bandpack.h"

typedef struct {
    int row;        /* bank row, -1: none (an empty chain)                */
    int start, len; /* first non-zero bin, bins up to the last non-zero   */
    int set, lane, t0; /* its weights: w{A,B}[(t0 + t) * 64 + lane]       */
    unsigned char d[32]; /* bins it starts early to sit on a bank pair    */
} PackRow;

typedef struct {
    int first, parts, cap; /* first partition, partitions, their taps     */
    int key;               /* shuffles chains of one capacity             */
    int idx;               /* its place before the sort: the last tie-break */
    int r;                 /* index into the rows                         */
    int lane, base;
} PackChain;

static unsigned pack_rand(unsigned *s) {
    /* the 32-bit linear congruential step, in 64 bits and masked: no product or sum wraps */
    *s = (unsigned)(((unsigned long long)*s * 1664525ull + 1013904223ull) & 0xffffffffull);
    return *s >> 8;
}

static int pack_need(const PackRow *r) { return r->row < 0 ? 0 : r->len + (r->start & 1); }

static int cmp_need_desc(const void *a, const void *b) {
    const PackRow *x = (const PackRow *)a, *y = (const PackRow *)b;
    const int nx = pack_need(x), ny = pack_need(y);
    if (nx != ny) return ny - nx;
    return x->row - y->row;
}

static int cmp_cap_desc(const void *a, const void *b) {
    const PackChain *x = (const PackChain *)a, *y = (const PackChain *)b;
    if (x->cap != y->cap) return y->cap - x->cap;
    if (x->key != y->key) return x->key - y->key;
    return x->idx - y->idx; /* a total order: the plan does not depend on how qsort treats ties */
}

/* the chain's base when its first slot sits on bank pair `residue`, -1 when its row does not allow that */
static int chain_base(const PackChain *c, const PackRow *r, int residue, int rowCap) {
    if (r->row < 0) return 2 * residue;
    const int d = r->d[residue];
    if (d > r->start || r->len + d > c->cap || r->start - d + c->cap > rowCap) return -1;
    return r->start - d;
}

static int kuhn_try(int u, int m, char adj[64][64], int *owner, char *seen, int rot) {
    for (int k = 0; k < m; k++) {
        const int s = (k + rot) % m;
        if (!adj[u][s] || seen[s]) continue;
        seen[s] = 1;
        if (owner[s] < 0 || kuhn_try(owner[s], m, adj, owner, seen, rot)) {
            owner[s] = u;
            return 1;
        }
    }
    return 0;
}

/* One partition: the chains list[0..n) against the slots (slotHalf, slotRes)[0..m), n <= m <= 64; openLane[h][..] are the lanes
 * of half h that the partition may still fill.  Returns 0, or 1 when an unmatched chain has no legal base at all. */
static int pack_stage(PackChain *ch, const PackRow *rows, const int *list, int n, const int *slotHalf, const int *slotRes, int m,
                      int openLane[2][32], const int *nOpen, int rowCap, unsigned *seed) {
    char adj[64][64];
    int owner[64], used[2] = {0, 0}, slotOf[64];
    for (int u = 0; u < n; u++)
        for (int s = 0; s < m; s++) adj[u][s] = chain_base(&ch[list[u]], &rows[ch[list[u]].r], slotRes[s], rowCap) >= 0;
    for (int s = 0; s < m; s++) owner[s] = -1;
    for (int u = 0; u < n; u++) slotOf[u] = -1;
    const int rot = m ? (int)(pack_rand(seed) % (unsigned)m) : 0;
    for (int u = 0; u < n; u++) {
        char seen[64];
        memset(seen, 0, sizeof(seen));
        kuhn_try(u, m, adj, owner, seen, rot);
    }
    for (int s = 0; s < m; s++)
        if (owner[s] >= 0) slotOf[owner[s]] = s;
    for (int u = 0; u < n; u++) {
        if (slotOf[u] < 0) continue;
        PackChain *c = &ch[list[u]];
        const int h = slotHalf[slotOf[u]];
        if (used[h] >= nOpen[h]) return 1;
        c->lane = openLane[h][used[h]++];
        c->base = chain_base(c, &rows[c->r], slotRes[slotOf[u]], rowCap);
    }
    for (int u = 0; u < n; u++) {
        if (slotOf[u] >= 0) continue;
        PackChain *c = &ch[list[u]];
        const PackRow *r = &rows[c->r];
        const int h = used[0] < nOpen[0] ? 0 : 1;
        if (used[h] >= nOpen[h]) return 1;
        c->lane = openLane[h][used[h]++];
        c->base = r->start - (r->start & 1);
        if (c->base + c->cap > rowCap) return 1;
    }
    return 0;
}

/* lane pairs of a half that meet on a bank pair within a partition's reads */
static int pack_conflicts(int base[3][64]) {
    int pairs = 0;
    for (int p = 0; p < 3; p++)
        for (int h = 0; h < 2; h++) {
            int cnt[32];
            memset(cnt, 0, sizeof(cnt));
            for (int l = 32 * h; l < 32 * h + 32; l++) cnt[(base[p][l] / 2) & 31]++;
            for (int r = 0; r < 32; r++) pairs += cnt[r] * (cnt[r] - 1) / 2;
        }
    return pairs;
}

/* the chains of (x, y, z) in dealing order, roomiest first; returns 1 when they hold the rows (sorted by need) */
static int pack_deal(PackChain *ch, const PackRow *rows, const int *t, int x, int y, int z, unsigned *seed) {
    const int a = t[0], b = t[1], c = t[2];
    const int first[6] = {0, 0, 0, 1, 1, 2}, parts[6] = {3, 2, 1, 2, 1, 1};
    const int cap[6] = {a + b + c, a + b, a, b + c, b, c}, cnt[6] = {x, y, x + z, z, x, x + y};
    int n = 0;
    for (int k = 0; k < 6; k++)
        for (int i = 0; i < cnt[k]; i++, n++) {
            ch[n].first = first[k], ch[n].parts = parts[k], ch[n].cap = cap[k];
            ch[n].key = seed ? (int)(pack_rand(seed) & 0xffff) : n;
            ch[n].idx = n;
            ch[n].lane = ch[n].base = -1;
        }
    qsort(ch, 128, sizeof(PackChain), cmp_cap_desc);
    for (int i = 0; i < 128; i++) {
        ch[i].r = i;
        if (pack_need(&rows[i]) > ch[i].cap) return 0;
    }
    if (seed) /* rows of nearly the same length change places where both still fit */
        for (int k = 0; k < 64; k++) {
            const int i = (int)(pack_rand(seed) % 127u);
            if (pack_need(&rows[ch[i].r]) <= ch[i + 1].cap && pack_need(&rows[ch[i + 1].r]) <= ch[i].cap) {
                const int tmp = ch[i].r;
                ch[i].r = ch[i + 1].r, ch[i + 1].r = tmp;
            }
        }
    return 1;
}

/* one try: fills cover[p][lane] = chain; returns the conflicting lane pairs, or -1 */
static int pack_try(PackChain *ch, const PackRow *rows, const int *t, int rowCap, unsigned *seed, int cover[3][64], int base[3][64]) {
    int list[64], slotHalf[64], slotRes[64], openLane[2][32], nOpen[2];
    for (int p = 0; p < 3; p++) {
        int n = 0, m = 0;
        for (int i = 0; i < 128; i++)
            if (ch[i].first == p) list[n++] = i;
        /* shuffle the order in which the chains ask */
        for (int i = n - 1; i > 0; i--) {
            const int j = (int)(pack_rand(seed) % (unsigned)(i + 1)), tmp = list[i];
            list[i] = list[j], list[j] = tmp;
        }
        for (int h = 0; h < 2; h++) {
            char busy[32];
            memset(busy, 0, sizeof(busy));
            nOpen[h] = 0;
            for (int l = 32 * h; l < 32 * h + 32; l++) {
                const int prev = p ? cover[p - 1][l] : -1;
                if (prev >= 0 && ch[prev].first + ch[prev].parts > p) {
                    cover[p][l] = prev;
                    base[p][l] = base[p - 1][l] + t[p - 1];
                    busy[(base[p][l] / 2) & 31] = 1;
                } else {
                    openLane[h][nOpen[h]++] = l;
                }
            }
            int free_ = 0;
            for (int r = 0; r < 32 && free_ < nOpen[h]; r++)
                if (!busy[r]) slotHalf[m] = h, slotRes[m] = r, m++, free_++;
        }
        if (n != nOpen[0] + nOpen[1] || m < n) return -1;
        if (pack_stage(ch, rows, list, n, slotHalf, slotRes, m, openLane, nOpen, rowCap, seed)) return -1;
        for (int i = 0; i < n; i++) {
            cover[p][ch[list[i]].lane] = list[i];
            base[p][ch[list[i]].lane] = ch[list[i]].base;
        }
    }
    return pack_conflicts(base);
}

void afx_bandpack_free(AfxBandPack *p) {
    if (!p) return;
    free(p->w);
    p->w = NULL;
}

int afx_bandpack_build(const AfxBandPlan *plan, const int (*layouts)[3], int n, int rowCap, int curSlots, AfxBandPack *out) {
    memset(out, 0, sizeof(*out));
    if (!plan || plan->split || plan->num <= 64 || plan->num > 128 || !plan->wA || !plan->wB || n < 1) return 1;
    PackRow rows[128];
    int nr = 0, longest = 0;
    for (int set = 0; set < 2; set++)
        for (int l = 0; l < 64; l++) {
            const int row = set ? plan->rowB[l] : plan->rowA[l], taps = set ? plan->tapsB : plan->tapsA;
            const float *w = set ? plan->wB : plan->wA;
            if (row < 0) continue;
            if (nr == 128) return 1;
            int f = -1, last = -1;
            for (int k = 0; k < taps; k++)
                if (w[(size_t)k * 64 + l] != 0.f) {
                    if (f < 0) f = k;
                    last = k;
                }
            PackRow *r = &rows[nr++];
            r->row = row, r->set = set, r->lane = l;
            r->t0 = f < 0 ? 0 : f;
            r->len = f < 0 ? 0 : last - f + 1;
            r->start = (set ? plan->startB[l] : plan->startA[l]) + r->t0;
            if (pack_need(r) > longest) longest = pack_need(r);
        }
    if (nr != plan->num) return 1;
    for (; nr < 128; nr++) rows[nr].row = -1, rows[nr].start = rows[nr].len = rows[nr].set = rows[nr].lane = rows[nr].t0 = 0;
    qsort(rows, 128, sizeof(PackRow), cmp_need_desc);
    for (int i = 0; i < 128; i++)
        for (int res = 0; res < 32; res++) rows[i].d[res] = (unsigned char)(((rows[i].start - 2 * res) % 64 + 64) % 64);

    /* layouts from the fewest slots */
    int order[16];
    if (n > 16) n = 16;
    for (int i = 0; i < n; i++) order[i] = i;
    for (int i = 1; i < n; i++)
        for (int j = i; j > 0; j--) {
            const int *u = layouts[order[j]], *v = layouts[order[j - 1]];
            if (u[0] + u[1] + u[2] >= v[0] + v[1] + v[2]) break;
            const int tmp = order[j];
            order[j] = order[j - 1], order[j - 1] = tmp;
        }
    for (int li = 0; li < n; li++) {
        const int *t = layouts[order[li]];
        const int slots = t[0] + t[1] + t[2];
        if (t[0] < 4 || t[1] < 4 || t[2] < 4 || ((t[0] | t[1] | t[2]) & 3) || slots < longest) continue;
        if (slots >= curSlots) break;
        /* candidates (x, y): every division of the lanes whose chains hold the rows, the roomiest first */
        enum { MAXC = 8, TRIES = 48 }; /* 384 tries: about 50 ms for 128 rows when none ends without a pair */
        int candX[MAXC], candY[MAXC], candS[MAXC], nc = 0;
        PackChain ch[128];
        for (int x = 0; x <= 32; x++)
            for (int y = 0; y <= 64 - 2 * x; y++) {
                if (!pack_deal(ch, rows, t, x, y, 64 - 2 * x - y, NULL)) continue;
                int score = 0;
                for (int i = 0; i < 128; i++) {
                    const int opt = (ch[i].cap - pack_need(&rows[ch[i].r])) / 2 + 1;
                    score += opt < 6 ? opt : 6;
                }
                int at;
                if (nc < MAXC) at = nc++;
                else if (score > candS[MAXC - 1]) at = MAXC - 1;
                else continue;
                while (at > 0 && candS[at - 1] < score) {
                    candX[at] = candX[at - 1], candY[at] = candY[at - 1], candS[at] = candS[at - 1];
                    at--;
                }
                candX[at] = x, candY[at] = y, candS[at] = score;
            }
        if (!nc) continue;
        int best = -1, bestCover[3][64], bestBase[3][64];
        PackChain bestCh[128];
        unsigned seed = 2024u;
        for (int k = 0; k < TRIES * nc && best != 0; k++) {
            const int ci = k % nc;
            int cover[3][64], base[3][64];
            if (!pack_deal(ch, rows, t, candX[ci], candY[ci], 64 - 2 * candX[ci] - candY[ci], k < nc ? NULL : &seed)) continue;
            const int got = pack_try(ch, rows, t, rowCap, &seed, cover, base);
            if (got >= 0 && (best < 0 || got < best)) {
                best = got;
                memcpy(bestCover, cover, sizeof(cover));
                memcpy(bestBase, base, sizeof(base));
                memcpy(bestCh, ch, sizeof(ch));
            }
        }
        /* a pair that meets on a bank pair serialises one partition's reads of a half (up to 12 ds_read_b64), about what a third
         * of the 12 removed reads bought: with more than one the packed plan has not been shown to gain, so the next layout
         * is tried, or the plan stays as it came */
        if (best < 0 || best > AFX_BANDPACK_MAX_PAIRS) continue;
        out->w = (float *)calloc((size_t)slots * 64, sizeof(float));
        if (!out->w) return 1;
        out->num = plan->num;
        out->taps[0] = t[0], out->taps[1] = t[1], out->taps[2] = t[2];
        out->slots = slots;
        out->conflicts = best;
        const int off[3] = {0, t[0], t[0] + t[1]};
        for (int l = 0; l < 64; l++)
            for (int p = 0; p < 3; p++) {
                const PackChain *c = &bestCh[bestCover[p][l]];
                const PackRow *r = &rows[c->r];
                out->base[p][l] = bestBase[p][l];
                out->cont[p][l] = c->first < p;
                out->row[p][l] = c->first + c->parts - 1 == p ? r->row : -1;
                if (c->first != p || r->row < 0) continue;
                const float *w = r->set ? plan->wB : plan->wA;
                const int d = r->start - c->base;
                for (int k = 0; k < r->len; k++) out->w[(size_t)(off[p] + d + k) * 64 + l] = w[(size_t)(r->t0 + k) * 64 + r->lane];
            }
        return 0;
    }
    return 1;
}
