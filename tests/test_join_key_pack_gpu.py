"""mdb_dev_join_key_pack (include/mdb_dev.h): one side of a composite join key, against the numpy restatement below, bit for bit -
the keys, every word of the NULL bitmap including the zero bits behind row n, the count of rows without a key - and nothing written
outside out_key[0 .. n) and the (n + 63) / 64 bitmap words (sentinel-filled margins around both)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_ROW = 0xFFFFFFFF
I64_MIN, I64_MAX = -2**63, 2**63 - 1
KEY_SENTINEL = -0x0123456789ABCDEF
BIT_SENTINEL = 0x5A5A5A5A5A5A5A5A
MARGIN = 66		# words in front of and behind each output


def np_pack(lay, cols, n):
    """cols: [(values int64[m], null flags bool[m] or None, rid uint32[n] or None)] in the layout's order -> (keys uint64[n], no-key flags bool[n])"""
    key = np.zeros(n, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    for c, (vals, nulls, rid) in enumerate(cols):
        row = np.arange(n, dtype=np.int64) if rid is None else rid.astype(np.int64)
        absent = row == NO_ROW
        safe = np.where(absent, 0, row)
        v = vals[safe] if n else np.zeros(0, dtype=np.int64)
        lo, span, shift = lay["lo"][c], lay["span"][c], lay["shift"][c]
        inside = (v >= lo) & (v <= lo + span)		# (lo + span is an int64: the larger of the two sides' maxima at most)
        bad |= absent | ~inside
        if nulls is not None:
            bad |= nulls[safe] & ~absent
        d = v.view(np.uint64) - np.uint64(lo % 2**64)	# modulo 2^64
        key |= np.where(inside, d, np.uint64(0)) << np.uint64(shift)
    key[bad] = 0
    return key, bad


def run_pack(dev, lay, cols, n, key_offset=0, in_offset=0):
    """packs on the device into sentinel-framed buffers and compares everything.  key_offset / in_offset 1: out_key / the rid-less value
    columns start 8 bytes off a 16-byte boundary (the kernel's 8-byte forms)"""
    import torch
    from midoridb_amd import dev as D
    words = (n + 63) // 64
    d_cols, keep = [], []
    for vals, nulls, rid in cols:
        if rid is None and in_offset:
            buf = dev.to_dev(np.concatenate([np.zeros(in_offset, dtype=np.int64), vals]))
            keep.append(buf)
            dv = buf[in_offset:]
        else:
            dv = dev.to_dev(vals)
        d_cols.append((dv, None if nulls is None else dev.nullbits_dev(nulls), None if rid is None else dev.to_dev(rid.astype(np.uint32))))
    kbuf = torch.full((MARGIN + key_offset + n + MARGIN,), KEY_SENTINEL, dtype=torch.int64, device=dev.device)
    bbuf = torch.full((MARGIN + words + MARGIN,), BIT_SENTINEL, dtype=torch.int64, device=dev.device)
    k0 = MARGIN + key_offset
    assert (kbuf.data_ptr() + 8 * k0) % 16 == 8 * (key_offset % 2)
    key, bits, nulls = dev.join_key_pack(lay, d_cols, n, out_key=kbuf[k0:k0 + max(n, 1)], out_nullbits=bbuf[MARGIN:MARGIN + max(words, 1)])
    e_key, e_bad = np_pack(lay, cols, n)
    h_k, h_b = kbuf.cpu().numpy(), bbuf.cpu().numpy()
    assert np.all(h_k[:k0] == KEY_SENTINEL) and np.all(h_k[k0 + n:] == KEY_SENTINEL), "out_key: written outside [0, n)"
    assert np.all(h_b[:MARGIN] == BIT_SENTINEL) and np.all(h_b[MARGIN + words:] == BIT_SENTINEL), "bitmap: written outside its words"
    assert np.array_equal(h_k[k0:k0 + n].view(np.uint64), e_key)
    assert np.array_equal(h_b[MARGIN:MARGIN + words].view(np.uint64), D.pack_nullbits(e_bad)[:words])	# (tail bits of the last word: 0)
    assert nulls == int(e_bad.sum())
    assert key.numel() == n and bits.numel() == words
    if n:
        assert int(e_key.max()) < 2**63
    return e_key, e_bad


def edge_values(rng, m, lo, hi):
    """m values of [lo - 1, hi + 1] (clipped to int64): mostly inside, the two ends and their outside neighbours for sure"""
    v = rng.integers(lo, hi, m, dtype=np.int64, endpoint=True)
    edges = [lo, hi, max(lo - 1, I64_MIN), min(hi + 1, I64_MAX)]
    for i, e in enumerate(edges * 2):
        if m:
            v[(i * 7919) % m] = e
    return v


def table_cols(rng, ncols, m, ranges, null_cols):
    out = []
    for c in range(ncols):
        v = edge_values(rng, m, *ranges[c])
        out.append((v, (rng.random(m) < 0.1) if c in null_cols else None))
    return out


RANGES = [(-5, 2), (10**12, 10**12 + 4999), (-2**40, -2**40 + 99_999), (7, 7)]		# negative lo, a far window, a large negative lo, one value


@pytest.mark.parametrize("ntaken", [2, 3, 4])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 300_001])
def test_pack_against_numpy(dev, n, ntaken):
    from midoridb_amd.dev import join_key_layout
    rng = np.random.default_rng(100 * n + ntaken)
    ranges = RANGES[:ntaken]
    lay = join_key_layout(ranges, ranges)
    assert lay["ntaken"] == ntaken and lay["lo"][0] == -5
    # 1. no row-id vector anywhere; NULL bits on none / on every second column
    for null_cols in ((), (0, 2)):
        t = table_cols(rng, ntaken, n, ranges, null_cols)
        e_key, e_bad = run_pack(dev, lay, [(v, nb, None) for v, nb in t], n)
        if n >= 4097 and not null_cols:
            assert 0 < e_bad.sum() < n // 2		# (the values outside, and only they)
            # exactly lo and lo + span pack to field values 0 and span
            v0 = t[0][0]
            ok = ~e_bad
            assert np.all((e_key[ok & (v0 == -5)] >> np.uint64(lay["shift"][0])) == 0)
            assert np.all((e_key[ok & (v0 == 2)] >> np.uint64(lay["shift"][0])) == 7)
    # ... from buffers that are 8 bytes off a 16-byte boundary (inputs, output, both)
    t = table_cols(rng, ntaken, n, ranges, (1,))
    for ko, io in ((1, 0), (0, 1), (1, 1)):
        run_pack(dev, lay, [(v, nb, None) for v, nb in t], n, key_offset=ko, in_offset=io)
    # 2. every column through ONE row-id vector with repeats and "no row"
    m = max(n // 3, 5)
    t = table_cols(rng, ntaken, m, ranges, (1,))
    rid = rng.integers(0, m, n, dtype=np.int64)
    gone = rng.random(n) < 0.05
    if n:
        gone[[0, n - 1, n // 2]] = [True, n > 64, True]
    rid = np.where(gone, NO_ROW, rid)
    e_key, e_bad = run_pack(dev, lay, [(v, nb, rid) for v, nb in t], n)
    assert np.all(e_bad[gone])
    # 3. mixed: column 0 through a row-id vector, column 1 as it stands, the others through a second vector without "no row"
    rid2 = rng.integers(0, m, n, dtype=np.int64)
    s = table_cols(rng, ntaken, n, ranges, (1, 3))
    cols = [(t[0][0], t[0][1], rid), (s[1][0], s[1][1], None)] + [(t[c][0], t[c][1], rid2) for c in range(2, ntaken)]
    run_pack(dev, lay, cols, n, key_offset=n % 2)
    # 4. one vector per column (as many distinct vectors as the layout has columns)
    rids = [rng.integers(0, m, n, dtype=np.int64) for _ in range(ntaken)]
    run_pack(dev, lay, [(t[c][0], t[c][1], rids[c]) for c in range(ntaken)], n)


@pytest.mark.parametrize("n", [65, 4097])
def test_superset_ranges_and_one_sided_intersection(dev, n):
    """the ranges the layout was made from are wider than the data on one side and narrower on the other: the field is their intersection,
    rows outside it get no key, rows inside pack relative to the intersection's lo"""
    from midoridb_amd.dev import join_key_layout
    rng = np.random.default_rng(n)
    lay = join_key_layout([(-1000, 1000), (0, 100)], [(-10, 5000), (50, 200)])
    assert lay["lo"] == [-10, 50] and lay["span"] == [1010, 50]
    a = [(rng.integers(-200, 201, n, dtype=np.int64), None, None), (rng.integers(40, 61, n, dtype=np.int64), rng.random(n) < 0.2, None)]
    e_key, e_bad = run_pack(dev, lay, a, n)
    assert e_bad.any() and not e_bad.all()
    # stale statistics that are wider than anything stored: nothing is outside, only NULLs lose their key
    lay = join_key_layout([(-10**6, 10**6), (-10**6, 10**6)], [(-10**6, 10**6), (-10**6, 10**6)])
    e_key, e_bad = run_pack(dev, lay, a, n)
    assert np.array_equal(e_bad, a[1][1])
    b = [(a[0][0], None, None), (a[1][0], None, None)]
    assert run_pack(dev, lay, b, n)[1].sum() == 0


@pytest.mark.parametrize("n", [64, 4097])
def test_63_bit_layout_at_the_ends_of_the_number_line(dev, n):
    """column 0 in [INT64_MIN, INT64_MIN + 2^31), column 1 in (INT64_MAX - 2^32, INT64_MAX]: 31 + 32 bits; values from the far end of
    the number line (whose distance to lo wraps modulo 2^64) are outside, the largest key is 2^63 - 1"""
    from midoridb_amd.dev import join_key_layout
    rng = np.random.default_rng(63 + n)
    r0, r1 = (I64_MIN, I64_MIN + 2**31 - 1), (I64_MAX - 2**32 + 1, I64_MAX)
    lay = join_key_layout([r0, r1], [r0, r1])
    assert lay["bits"] == [31, 32] and lay["total_bits"] == 63
    v0 = rng.integers(r0[0], r0[1], n, dtype=np.int64, endpoint=True)
    v1 = rng.integers(r1[0], r1[1], n, dtype=np.int64, endpoint=True)
    v0[:8] = [r0[0], r0[1], r0[1] + 1, I64_MAX, 0, -1, r0[1], r0[0]]
    v1[:8] = [r1[0], r1[1], r1[1], r1[1], r1[0], r1[0], r1[0] - 1, I64_MIN]
    v0[8:12] = [r0[1], r0[0], I64_MAX - 5, r0[1]]
    v1[8:12] = [r1[1], 0, r1[1], I64_MIN + 5]
    e_key, e_bad = run_pack(dev, lay, [(v0, None, None), (v1, None, None)], n)
    assert e_bad[:12].tolist() == [False, False, True, True, True, True, True, True, False, True, True, True]
    assert int(e_key[0]) == 0 and int(e_key[1]) == 2**63 - 1 and int(e_key[8]) == 2**63 - 1
    rid = rng.integers(0, n, n, dtype=np.int64)
    rid[::9] = NO_ROW
    run_pack(dev, lay, [(v0, None, rid), (v1, rng.random(n) < 0.3, rid)], n, key_offset=1)


def test_refusals(dev):
    """a layout that serves nothing (fewer than two columns, or empty) is an error, not a launch"""
    import torch
    from midoridb_amd.dev import DeviceError, join_key_layout
    v = torch.zeros(8, dtype=torch.int64, device=dev.device)
    one = join_key_layout([(0, 2**32 - 1), (0, 2**32 - 1)], [(0, 2**32 - 1), (0, 2**32 - 1)])
    assert one["ntaken"] == 1
    with pytest.raises(DeviceError):
        dev.join_key_pack(one, [(v, None, None)], 8)
    empty = join_key_layout([(0, 5), (0, 5)], [(0, 5), (6, 9)])
    assert empty["empty"] == 1 and empty["ntaken"] == 2
    with pytest.raises(DeviceError):
        dev.join_key_pack(empty, [(v, None, None), (v, None, None)], 8)
