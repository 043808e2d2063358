"""CPU: tests/shred_lib.py's restatement of the shred Merkle root and its flag
against the reference's roots in tests/golden/shred_roots.npz, and the flag's
reject classes and boundaries (the GPU tests then hold the engine to
shred_lib and the fixture)."""
import numpy as np
import pytest

import shred_lib as S


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


def test_roots_equal_reference(golden):
    shreds, roots = S.golden_shreds(golden)
    assert len(shreds) == len(roots) >= 128 + 150
    for i, s in enumerate(shreds):
        flag, root = S.shred_root(s)
        assert flag == 1, i
        assert root == bytes(roots[i]), i


def test_fixture_covers_types_and_depths(golden):
    """every Merkle type x depth 0..9 with the lowest, the highest and a middle
    tree index.  A code shred's tree index is code.idx + data_cnt >= 1, so no
    code shred of depth 0 has a root: those three pairs cannot be in it."""
    seen = {}
    for i in range(len(golden["syn_sz"])):
        b = bytes(golden["syn"][i])
        v = b[S.OFF_VARIANT]
        data = (v & 0xC0) == 0x80
        if data:
            t = (int.from_bytes(b[S.OFF_IDX:S.OFF_IDX + 4], "little") - int.from_bytes(b[S.OFF_FEC_SET_IDX:S.OFF_FEC_SET_IDX + 4], "little")) & 0xffffffff
        else:
            t = int.from_bytes(b[S.OFF_CODE_IDX:S.OFF_CODE_IDX + 2], "little") + int.from_bytes(b[S.OFF_DATA_CNT:S.OFF_DATA_CNT + 2], "little")
        seen.setdefault((v & 0xf0, v & 0x0f), set()).add(t)
    for typ in S.MERKLE_TYPES:
        data = typ in S.DATA_TYPES
        for d in range(10):
            if not data and d == 0:
                assert (typ, d) not in seen
                continue
            lo = 0 if data else 1
            hi = min((1 << d) - 1, 66 if data else 133)
            got = seen[(typ, d)]
            assert lo in got and hi in got, (hex(typ), d, got)
            assert hi - lo < 2 or any(lo < t < hi for t in got), (hex(typ), d, got)


def test_shredder_sets_have_one_root(golden):
    assert golden["set"].shape == (2, 64, S.MAX_SZ)
    for s in range(2):
        assert (golden["set_sz"][s, :32] == S.MIN_SZ).all() and (golden["set_sz"][s, 32:] == S.MAX_SZ).all()
        assert (golden["set_root"][s] == golden["set_root"][s, 0]).all()
        assert golden["set_root"][s].any()
    assert (golden["set_root"][0, 0] != golden["set_root"][1, 0]).any()
    # every shred of a set carries the same signature
    for s in range(2):
        assert (golden["set"][s, :, :64] == golden["set"][s, 0, :64]).all()


def test_flag_rejects_and_boundaries():
    for name, shred, want in S.reject_cases(np.random.default_rng(7)):
        flag, root = S.shred_root(shred)
        assert flag == want, name
        assert (root == bytes(32)) == (want == 0), name


def test_nothing_past_sz_is_interpreted():
    """a rejected short shred's verdict does not depend on the bytes after it"""
    rng = np.random.default_rng(8)
    s = S.make_shred(rng, 0x40, 7, 40, sz=1228)
    assert S.shred_root(s)[0] == 1 and S.shred_root(s[:1227])[0] == 0
    pool, off, sz = S.pack([s[:1227], s])
    flags, roots = S.shred_roots(pool, off, sz)
    assert list(flags) == [0, 1] and not roots[0].any() and roots[1].any()
