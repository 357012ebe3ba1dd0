#!/usr/bin/env python3
"""Where the wave slots of a k_stft_mel_v2 launch stand empty: reads the stamp file of a -DAFX_V2_STAMPS build of
afx_melfused2.hip (AFX_V2_STAMPS_FILE; one record of 64 u64 per wave: s_memtime at the first frame, after the last, workgroup | wave
<< 32, frames, HW_ID, XCC_ID, -, -, then one stamp per 16 frames done) and prints

  * per workgroup: the spread between its first and its last finishing wave as a share of the workgroup's duration, and the share
    of its twelve wave slots' time that is empty before the first frame and after the last one of a wave;
  * per CU (XCC_ID, SE_ID, SH_ID, CU_ID of HW_ID): the time between workgroups, and the CU's span from its first wave's start to
    its last wave's end against the longest span of any CU (stamps of two CUs are never compared with each other);
  * W3: wave-cycles per frame over the window of a workgroup in which all its waves are running (12 x window / frames done in the
    window, frames between two stamps spread evenly), median over workgroups;
  * the split of all empty slot time into inside workgroups / between workgroups / end of launch.

Stamps cost time of their own: read shares, not speed.

    python tools/v2_stamps.py STAMPS.bin [label]"""
import sys

import numpy as np

WORDS, HEAD, WAVES = 64, 8, 12


def frames_done(rec, at):
    """frames of a wave done at time `at`: piecewise linear through (t0, 0), (stamp k, 16 k), (t1, n)"""
    n = int(rec[3])
    k = min(n // 16, WORDS - HEAD)
    ts = np.concatenate(([rec[0]], rec[HEAD:HEAD + k], [rec[1]])).astype(np.float64)
    fs = np.concatenate(([0], 16 * np.arange(1, k + 1), [n])).astype(np.float64)
    return float(np.interp(at, ts, fs))


def main():
    raw = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, WORDS)
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    raw = raw[raw[:, 3] > 0]  # waves that ran a frame
    wg = (raw[:, 2] & 0xFFFFFFFF).astype(np.int64)
    t0, t1, n = raw[:, 0].astype(np.float64), raw[:, 1].astype(np.float64), raw[:, 3].astype(np.int64)
    cu = ((raw[:, 5] & 0xF) << 8) | ((raw[:, 4] >> 8) & 0xFF)  # XCC_ID | SE_ID, SH_ID, CU_ID
    xcc = (raw[:, 5] & 0xF).astype(np.int64)
    print(f"== {label}: {len(raw)} waves with frames, {len(np.unique(wg))} workgroups, {int(n.sum())} frames, {len(np.unique(cu))} CUs seen on {len(np.unique(xcc))} XCDs")
    spread, empty_in, w3, per_wave = [], [], [], []
    groups = {}
    inside = 0.0
    for g in np.unique(wg):
        m = wg == g
        assert len(np.unique(cu[m])) == 1, "a workgroup on two CUs: the HW_ID fields are not what this tool takes them for"
        b, e = t0[m].min(), t1[m].max()
        dur = e - b
        spread.append((t1[m].max() - t1[m].min()) / dur)
        lost = (WAVES * dur - (t1[m] - t0[m]).sum())  # slots of waves that never ran a frame count as empty for the whole duration
        empty_in.append(lost / (WAVES * dur))
        inside += lost
        lo, hi = t0[m].max(), t1[m].min()
        if m.sum() == WAVES and hi > lo:
            done = sum(frames_done(r, hi) - frames_done(r, lo) for r in raw[m])
            if done > 0:
                w3.append(WAVES * (hi - lo) / done)
        per_wave.extend(((t1[m] - t0[m]) / n[m]).tolist())
        groups.setdefault(int(cu[m][0]), []).append((b, e))
    # s_memtime of two CUs is not compared: counters of different XCDs (and, as measured, of CUs within one) stand apart by far
    # more than a launch.  A CU's own span, first wave's start to last wave's end, needs one clock only; with all CUs started
    # together by the dispatcher, the longest span stands for the launch and a shorter one leaves its CU idle at the end
    between = 0.0
    gaps, spans = [], []
    for c, iv in groups.items():
        iv.sort()
        for (b0, e0), (b1, e1) in zip(iv, iv[1:]):
            gaps.append(max(b1 - e0, 0.0))
            between += WAVES * max(b1 - e0, 0.0)
        spans.append(iv[-1][1] - iv[0][0])
    spans = np.array(spans)
    window = spans.max()
    tails = window - spans
    tail = WAVES * tails.sum()
    slots = WAVES * len(groups) * window
    q = lambda a: "median %.4g mean %.4g max %.4g" % (np.median(a), np.mean(a), np.max(a)) if len(a) else "none"
    print(f"launch window (longest span of a CU) {window:.0f} ticks; workgroups per CU {np.mean([len(v) for v in groups.values()]):.2f}")
    print(f"per workgroup: last - first finishing wave / duration: {q(spread)}")
    print(f"per workgroup: empty share of its {WAVES} slots: {q(empty_in)}")
    print(f"per CU: gap between workgroups, ticks: {q(gaps)}; span, ticks: median {np.median(spans):.0f} min {spans.min():.0f} max {spans.max():.0f}; "
          f"idle at the end of the launch: {q(tails)} ({np.mean(tails) / window:.4f} of the window)")
    print(f"wave ticks per frame, whole life of a wave: {q(per_wave)}")
    print(f"W3, wave ticks per frame while all {WAVES} waves of a workgroup run: {q(w3)} over {len(w3)} workgroups")
    total = inside + between + tail
    print(f"empty slot time {total / slots:.4f} of all slot time: inside workgroups {inside / total:.3f}, between workgroups {between / total:.3f}, "
          f"end of launch {tail / total:.3f}")
    print(f"resident waves per SIMD from the stamps: {(t1 - t0).sum() / (4 * len(groups) * window):.3f} of {WAVES // 4}")


if __name__ == "__main__":
    main()
