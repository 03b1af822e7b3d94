"""mdb_dev_join_key_unpack (include/mdb_dev.h): packed composite keys back to their key columns, against the numpy restatement below,
bit for bit, with nothing written outside out_cols[c][0 .. n) (sentinel-filled margins around every output), and the round trip
pack -> unpack = the original cells for every row that has a key."""
import numpy as np
import pytest

from tests.test_join_key_pack_gpu import I64_MIN, KEY_SENTINEL, MARGIN, RANGES, np_pack, table_cols

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 127, 128, 129, 2047, 2048, 2049, 5000]		# (a workgroup takes 2048 keys, a wave 128, a lane 2)
# 63 bits in all, the first lo three above the smallest int64: 20 + 30 + 13 + 0 bits
RANGES_63 = [(I64_MIN + 3, I64_MIN + 3 + 2**20 - 1), (10**12, 10**12 + 2**30 - 1), (-2**40, -2**40 + 2**13 - 1), (7, 7)]


def np_unpack(lay, keys):
    """keys uint64[n] -> [int64[n]] * ntaken: lo_c + ((key >> shift_c) & (2^bits_c - 1)) modulo 2^64"""
    out = []
    for c in range(lay["ntaken"]):
        field = (keys >> np.uint64(lay["shift"][c])) & np.uint64((1 << lay["bits"][c]) - 1)
        out.append((field + np.uint64(lay["lo"][c] % 2**64)).view(np.int64))
    return out


def random_keys(rng, lay, n):
    """keys whose every field lies in [0, span_c], the two ends for sure"""
    key = np.zeros(n, dtype=np.uint64)
    for c in range(lay["ntaken"]):
        f = rng.integers(0, lay["span"][c], n, dtype=np.uint64, endpoint=True)
        if n:
            f[0], f[n - 1], f[n // 2] = 0, lay["span"][c], lay["span"][c]
        key |= f << np.uint64(lay["shift"][c])
    return key


def run_unpack(dev, lay, keys, key_offset=0, out_offset=None):
    """unpacks on the device into sentinel-framed buffers and compares everything.  key_offset 1: the keys start 8 bytes off a 16-byte
    boundary; out_offset c: so does output column c (the kernel's 8-byte forms)"""
    import torch
    n, nt = len(keys), lay["ntaken"]
    kbuf = dev.to_dev(np.concatenate([np.zeros(key_offset, dtype=np.int64), keys.view(np.int64), np.zeros(1, dtype=np.int64)]))
    dk = kbuf[key_offset:key_offset + max(n, 1)]
    assert dk.data_ptr() % 16 == 8 * key_offset
    bufs, outs, starts = [], [], []
    for c in range(nt):
        o0 = MARGIN + (1 if out_offset == c else 0)
        b = torch.full((o0 + n + MARGIN,), KEY_SENTINEL, dtype=torch.int64, device=dev.device)
        assert (b.data_ptr() + 8 * o0) % 16 == (8 if out_offset == c else 0)
        bufs.append(b)
        starts.append(o0)
        outs.append(b[o0:o0 + max(n, 1)])
    got = dev.join_key_unpack(lay, dk, n, out_cols=outs)
    exp = np_unpack(lay, keys)
    for c in range(nt):
        h = bufs[c].cpu().numpy()
        assert np.all(h[:starts[c]] == KEY_SENTINEL) and np.all(h[starts[c] + n:] == KEY_SENTINEL), f"column {c}: written outside [0, n)"
        assert np.array_equal(h[starts[c]:starts[c] + n], exp[c]), f"column {c}"
        assert got[c].numel() == n
    return exp


@pytest.mark.parametrize("ntaken", [2, 3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_unpack_against_numpy(dev, n, ntaken):
    from midoridb_amd.dev import join_key_layout
    rng = np.random.default_rng(1000 * n + ntaken)
    for ranges in (RANGES[:ntaken], RANGES_63[:ntaken]):
        lay = join_key_layout(ranges, ranges)
        assert lay["ntaken"] == ntaken and lay["lo"][0] == ranges[0][0]
        keys = random_keys(rng, lay, n)
        exp = run_unpack(dev, lay, keys)
        for c in range(ntaken if n else 0):	# both ends of every field come back exactly
            assert exp[c].max() == ranges[c][1] and (n < 2 or exp[c].min() == ranges[c][0])
        # the keys, one output, both 8 bytes off a 16-byte boundary
        run_unpack(dev, lay, keys, key_offset=1)
        run_unpack(dev, lay, keys, out_offset=ntaken - 1)
        run_unpack(dev, lay, keys, key_offset=1, out_offset=0)


def test_63_bit_layout_first_lo_near_int64_min(dev):
    from midoridb_amd.dev import join_key_layout
    lay = join_key_layout(RANGES_63, RANGES_63)
    assert lay["total_bits"] == 63 and lay["bits"] == [20, 30, 13, 0] and lay["lo"][0] == I64_MIN + 3
    keys = np.array([0, 2**63 - 1, 1 << 43, (1 << 43) - 1, 1 << 13, (1 << 13) - 1], dtype=np.uint64)
    exp = run_unpack(dev, lay, keys)
    assert [int(e[0]) for e in exp] == [I64_MIN + 3, 10**12, -2**40, 7]
    assert [int(e[1]) for e in exp] == [I64_MIN + 3 + 2**20 - 1, 10**12 + 2**30 - 1, -2**40 + 2**13 - 1, 7]


@pytest.mark.parametrize("ntaken", [2, 3, 4])
@pytest.mark.parametrize("n", [129, 2049, 5000])
def test_round_trip(dev, n, ntaken):
    """pack, then unpack: every row that has a key gets its original cells back (rows without one - a NULL cell, a value outside its
    field - pack to key 0, which unpacks to every lo)"""
    from midoridb_amd.dev import join_key_layout
    rng = np.random.default_rng(77 * n + ntaken)
    for ranges in (RANGES[:ntaken], RANGES_63[:ntaken]):
        lay = join_key_layout(ranges, ranges)
        t = table_cols(rng, ntaken, n, ranges, (1,))
        e_key, e_bad = np_pack(lay, [(v, nb, None) for v, nb in t], n)
        d_cols = [(dev.to_dev(v), None if nb is None else dev.nullbits_dev(nb), None) for v, nb in t]
        key, _, nulls = dev.join_key_pack(lay, d_cols, n)
        assert np.array_equal(key.cpu().numpy().view(np.uint64), e_key) and nulls == int(e_bad.sum()) and 0 < nulls < n
        back = dev.join_key_unpack(lay, key, n)
        for c in range(ntaken):
            got = back[c].cpu().numpy()
            assert np.array_equal(got[~e_bad], t[c][0][~e_bad]), f"column {c}"
            assert np.all(got[e_bad] == ranges[c][0])


def test_refusals_write_nothing(dev):
    """a layout that serves nothing (fewer than two columns, or empty) is an error, not a launch"""
    import torch
    from midoridb_amd.dev import DeviceError, join_key_layout
    keys = torch.zeros(8, dtype=torch.int64, device=dev.device)
    outs = [torch.full((8,), KEY_SENTINEL, dtype=torch.int64, device=dev.device) for _ in range(2)]
    one = join_key_layout([(0, 2**32 - 1), (0, 2**32 - 1)], [(0, 2**32 - 1), (0, 2**32 - 1)])
    assert one["ntaken"] == 1
    with pytest.raises(DeviceError):
        dev.join_key_unpack(one, keys, 8, out_cols=outs[:1])
    empty = join_key_layout([(0, 5), (0, 5)], [(0, 5), (6, 9)])
    assert empty["empty"] == 1 and empty["ntaken"] == 2
    with pytest.raises(DeviceError):
        dev.join_key_unpack(empty, keys, 8, out_cols=outs)
    for o in outs:
        assert bool((o == KEY_SENTINEL).all())
