"""numpy prototype of the reader-side W_64 twiddles of the fused kernel (afx_melfused2.hip, round 10): the index algebra of the
new table and of the stage-3 reads, and an LDS bank-conflict check per read class.

Change against tools/proto_fft1024_v2.py (which stays as the record of the other layouts):
  * the second radix-16 writes the exchange-2 image V[q = k1 + 16 j1][m2] WITHOUT the twiddle W_64^(m2 j1); the lane that
    reads a base q in stage 3 multiplies V[q][1..3] by row j1 = q >> 4 of a table of 16 rows:
        row j1 = [ W^(j1), W^(2 j1) | W^(3 j1), pad ]      (W = W_64; 32 bytes, two 16-byte halves)
    one ds_read_b128 (first half) + one ds_read_b64 (W^(3 j1)) per base; V[q][0] needs no twiddle
  * four bases per lane: own q = lane, lane + 64 (rows lane >> 4 and + 4), mirrors qm0 = 128 (lane 0) | 256 - lane and
    qm1 = 192 - lane; 12 complex products per lane where the writer side had 15, 4 + 4 reads where it had 8 ds_read_b128
"""
import numpy as np

N, M = 2048, 1024
TW2_PITCH = 32          # bytes per table row
lane = np.arange(64)

# read lane groups (MI355X LDS: ds_read_b128 4 x 16 non-contiguous lanes, ds_read_b64 2 x 32), 64 banks of 4 bytes
G128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
        [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G128 = G128 + [[l + 32 for l in g] for g in G128]
G64R = [list(range(0, 32)), list(range(32, 64))]


def conflicts(addr, width, groups, nbanks=64):
    """worst multiplicity of distinct addresses on one bank within a lane group (1 = conflict-free)"""
    worst = 1
    for g in groups:
        banks = {}
        for l in g:
            for d in range(width // 4):
                b = ((addr[l] + 4 * d) // 4) % nbanks
                banks.setdefault(b, set()).add(addr[l] + 4 * d)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def table_rows():
    """the table as complex128 [16][4] (pad = 0): entry (j, m - 1) = W_64^(m j)"""
    t = np.zeros((16, 4), complex)
    for j in range(16):
        for m in (1, 2, 3):
            t[j, m - 1] = np.exp(-2j * np.pi * (m * j) / 64.0)
    return t


def bases():
    """the four bases of every lane: (s = 0 own, s = 0 mirror, s = 1 own, s = 1 mirror)"""
    qm0 = np.where(lane == 0, 128, 256 - lane)
    qm1 = 192 - lane
    return lane, qm0, lane + 64, qm1


def read_classes():
    """byte addresses (table-relative) of the eight stage-3 table reads: name -> (addresses, width)"""
    out = {}
    for name, q in zip(("own s=0", "mirror s=0", "own s=1", "mirror s=1"), bases()):
        row = q >> 4
        assert row.min() >= 0 and row.max() <= 15
        out[name + " b128"] = (TW2_PITCH * row, 16)
        out[name + " b64"] = (TW2_PITCH * row + 16, 8)
    return out


def check_banks(pitch=TW2_PITCH):
    """no lane group of any class meets a bank twice; returns {class: worst multiplicity}"""
    res = {}
    for name, (addr, width) in read_classes().items():
        addr = addr // TW2_PITCH * pitch + addr % TW2_PITCH
        res[name] = conflicts(addr, width, G128 if width == 16 else G64R)
    return res


def check_rows():
    """the rows the issue lists: own bases rows lane >> 4 and + 4; mirrors rows 8 and 12-15, and rows 8-12"""
    q0, qm0, q1, qm1 = bases()
    assert np.all((q0 >> 4) == (lane >> 4)) and np.all((q1 >> 4) == (lane >> 4) + 4)
    assert set((qm0 >> 4).tolist()) == {8, 12, 13, 14, 15} and (qm0[0] >> 4) == 8
    assert set((qm1 >> 4).tolist()) == {8, 9, 10, 11, 12}


def transform(x, reader_side=True):
    """the packed 1024-point transform of 2048 real samples through both exchanges (float64): rfft bins 0 .. 1024"""
    z = x[0::2] + 1j * x[1::2]
    a = np.stack([z[64 * n1 + lane] for n1 in range(16)], axis=1)
    Y = np.fft.fft(a, axis=-1) * np.exp(-2j * np.pi * np.outer(lane, np.arange(16)) / M)
    k1, m2 = lane >> 2, lane & 3
    b = np.zeros((64, 16), complex)
    for k in range(16):        # exchange 1: lane (m1, m2) holds Y[n2 = 4 m1 + m2][k]; reader (k1, m2) takes m1 = 0 .. 15
        for l in range(64):
            b[4 * k + (l & 3), l >> 2] = Y[l, k]
    V = np.fft.fft(b, axis=-1)  # V[lane (k1, m2)][j1]
    tab = table_rows()
    if not reader_side:
        V = V * np.exp(-2j * np.pi * np.outer(m2, np.arange(16)) / 64)
    img = np.zeros((256, 4), complex)   # image V[q][m2]
    for j1 in range(16):
        img[k1 + 16 * j1, m2] = V[:, j1]
    Z = np.zeros(M, complex)
    for q in range(256):
        r = img[q].copy()
        if reader_side:
            r[1:] = r[1:] * tab[q >> 4, :3]
        Z[q + 256 * np.arange(4)] = np.fft.fft(r)
    k = np.arange(M + 1)
    Zk, Zm = Z[k % M], np.conj(Z[(M - k) % M])
    return 0.5 * (Zk + Zm) - 0.5j * np.exp(-2j * np.pi * k / N) * (Zk - Zm)


def main():
    check_rows()
    for name, worst in check_banks().items():
        assert worst == 1, (name, worst)
    # (what the pitch must avoid: at 128 bytes rows r and r + 2 share their banks, at 256 every row does -- the mirror classes
    #  meet three consecutive rows in one lane group)
    assert max(check_banks(128).values()) == 2 and max(check_banks(256).values()) == 3
    x = np.random.default_rng(0).standard_normal(N)
    ref = np.fft.rfft(x)
    for rs in (False, True):
        X = transform(x, rs)
        assert np.allclose(X, ref), np.abs(X - ref).max()
    print("v3 layouts OK: max err", np.abs(transform(x) - ref).max())


if __name__ == "__main__":
    main()
