"""GPU: device SHA-256, shred Merkle roots and FEC-set verification from raw
shreds (include/fd_replay_hip.h, shred section) against hashlib, the
reference's roots in tests/golden/shred_roots.npz, tests/shred_lib.py and the
oracle's fd_ed25519_verify.  Every comparison is byte-exact."""
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import shred_lib as S
from firedancer_amd import ERRMODE_AVX512, ERRMODE_REF, FD_SHRED_HIP_NO_ROOT, ShredVerifier, replay

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
SMALL_ORDER = bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a")   # a point of order 8


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


@pytest.fixture(scope="module")
def golden():
    g = S.load_golden()
    shreds, roots = S.golden_shreds(g)
    return {"g": g, "shreds": shreds, "roots": roots}


def run_roots(verifier, shreds):
    import torch
    pool, off, sz = S.pack(shreds)
    n = len(shreds)
    roots = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    flags = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    assert replay.shred_roots_dev(verifier, n, _dev(pool), _dev(off), _dev(sz), roots, flags) == 0
    torch.cuda.synchronize()
    return flags.cpu().numpy(), roots.cpu().numpy()


# ---- 1. the SHA-256 core ------------------------------------------------------

def test_sha256_batch(verifier):
    import torch
    rng = np.random.default_rng(256)
    lens = [0, 1, 55, 56, 63, 64, 65, 119, 120, 1190] + [int(x) for x in rng.integers(0, 1301, 64)]
    msgs = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in lens]
    want = np.array([np.frombuffer(hashlib.sha256(m).digest(), np.uint8) for m in msgs])
    for n in (1, 63, 64, 65, len(msgs)):
        for shift in (0, 5):                      # message i at residue (i + shift) mod 16
            parts, off, o = [], [], 0
            for i in range(n):
                pad = (-o) % 16 + (i + shift) % 16
                parts.append(bytes(pad)); o += pad
                off.append(o); parts.append(msgs[i]); o += len(msgs[i])
            parts.append(bytes(32))
            if n >= 16:
                assert {x % 16 for x in off} == set(range(16))
            pool = np.frombuffer(b"".join(parts), np.uint8)
            out = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
            rc = replay.sha256_batch_dev(verifier, n, _dev(pool), _dev(np.array(off, np.uint32)),
                                         _dev(np.array(lens[:n], np.uint32)), out)
            torch.cuda.synchronize()
            assert rc == 0
            got = out.cpu().numpy()
            bad = np.nonzero((got != want[:n]).any(axis=1))[0]
            assert bad.size == 0, (n, shift, [(int(i), lens[i], off[i] % 16) for i in bad[:8]])


# ---- 2. roots -------------------------------------------------------------------

def test_roots_fixture(verifier, golden):
    shreds, roots = golden["shreds"], golden["roots"]
    rng = np.random.default_rng(2)
    for n in (len(shreds), 1, 63, 64, 65, 257):
        order = rng.permutation(len(shreds))[:n]  # data and code, and the depths, mixed within every wave
        flags, got = run_roots(verifier, [shreds[i] for i in order])
        assert (flags == 1).all(), (n, np.nonzero(flags != 1)[0][:8])
        bad = np.nonzero((got != roots[order]).any(axis=1))[0]
        assert bad.size == 0, (n, [(int(i), hex(shreds[order[i]][S.OFF_VARIANT])) for i in bad[:8]])


# ---- 3. rejects -----------------------------------------------------------------

def test_rejects_among_good(verifier, golden):
    cases = S.reject_cases(np.random.default_rng(7))
    assert sum(1 for c in cases if not c[2]) >= 17
    good = golden["shreds"]
    shreds, names = [], []
    for k in range(128):                          # two waves: every third shred is a case, the others good
        if k % 3 == 1 and k // 3 < len(cases):
            names.append(cases[k // 3][0]); shreds.append(cases[k // 3][1])
        else:
            names.append(None); shreds.append(good[(7 * k) % len(good)])
    assert names.count(None) == 128 - len(cases)
    want_f = np.array([S.shred_root(s)[0] for s in shreds], np.uint8)
    want_r = np.array([np.frombuffer(S.shred_root(s)[1], np.uint8) for s in shreds])
    for k, nm in enumerate(names):
        if nm is not None:
            assert want_f[k] == cases[k // 3][2]
    flags, roots = run_roots(verifier, shreds)
    assert [names[i] for i in np.nonzero(flags != want_f)[0]] == []
    assert not roots[want_f == 0].any()
    bad = np.nonzero((roots != want_r).any(axis=1))[0]
    assert [(int(i), names[i]) for i in bad] == []


# ---- 4. verify --------------------------------------------------------------------

def _signed(shred, root, prv):
    pub = O.public_from_private(prv)
    return O.sign(root, pub, prv) + shred[64:], pub


def verify_batch(golden):
    """(shreds, pubs): the two shredder sets, signed synthetic shreds three
    times each, the mutations and two shreds without a root, shuffled"""
    g = golden["g"]
    rng = np.random.default_rng(4)
    leader = bytes(g["leader"])
    sets = golden["shreds"][-128:]
    items = [(s, leader) for s in sets]
    syn = golden["shreds"][:len(g["syn_sz"])]
    for k in range(8):
        i = int(rng.integers(0, len(syn)))
        s, pub = _signed(syn[i], bytes(golden["roots"][i]), rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        items += [(s, pub)] * 3
    d0, c0, d1 = sets[3], sets[40], sets[64 + 9]
    flip = bytearray(d0); flip[17] ^= 0x04                                   # one signature bit
    items.append((bytes(flip), leader))
    items.append((c0, O.public_from_private(bytes(range(32)))))               # a wrong leader key
    pay = bytearray(d1); pay[300] ^= 0x01                                     # one payload byte: another root
    items.append((bytes(pay), leader))
    spl = bytearray(c0); spl[32:64] = (int.from_bytes(c0[32:64], "little") + L).to_bytes(32, "little")
    items.append((bytes(spl), leader))                                        # S + L
    items.append((d0, SMALL_ORDER))
    items.append((d0[:1202], leader))                                         # no root
    items.append((S.make_shred(rng, 0x80, 10, 5), leader))                    # no root
    # scatter: the repeats of a synthetic shred land in different waves of the 3
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    return [s for s, _ in items], [p for _, p in items]


def expected_codes(shreds, pubs, errmode):
    codes, triples = [], set()
    for s, p in zip(shreds, pubs):
        f, root = S.shred_root(s)
        if f:
            codes.append(O.verify(root, s[:64], p, errmode))
            triples.add((s[:64], root, p))
        else:
            codes.append(FD_SHRED_HIP_NO_ROOT)
    return np.array(codes, np.int8), len(triples)


def launch_verify(sv, shreds, pubs):
    """tensors in, the call queued, no sync: (roots, flags, codes) device tensors"""
    import torch
    pool, off, sz = S.pack(shreds)
    n = len(shreds)
    keep = (_dev(pool), _dev(off), _dev(sz), _dev(np.frombuffer(b"".join(pubs), np.uint8)))
    roots = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    flags = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    codes = torch.full((n,), 0x5A, dtype=torch.int8, device="cuda")
    sv.verify_dev(n, keep[0], keep[1], keep[2], keep[3], roots, flags, codes)
    return roots, flags, codes, keep


def check_verify(out, shreds, pubs, errmode):
    roots, flags, codes, _ = out
    want, _ = expected_codes(shreds, pubs, errmode)
    want_f = np.array([S.shred_root(s)[0] for s in shreds], np.uint8)
    want_r = np.array([np.frombuffer(S.shred_root(s)[1], np.uint8) for s in shreds])
    assert (flags.cpu().numpy() == want_f).all()
    assert (roots.cpu().numpy() == want_r).all()
    got = codes.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:10]]


@pytest.mark.parametrize("errmode", [ERRMODE_AVX512, ERRMODE_REF])
def test_verify(verifier, golden, errmode):
    import torch
    shreds, pubs = verify_batch(golden)
    want, distinct = expected_codes(shreds, pubs, errmode)
    assert {0, -1, -2, -3, FD_SHRED_HIP_NO_ROOT} <= set(int(c) for c in want)
    waves = {}
    for i, s in enumerate(shreds):
        waves.setdefault(s, set()).add(i // 64)
    assert sum(1 for s, w in waves.items() if shreds.count(s) == 3 and len(w) > 1) >= 1
    sv = ShredVerifier(verifier, 256)
    verifier.set_errmode(errmode)
    try:
        out = launch_verify(sv, shreds, pubs)
        torch.cuda.synchronize()
        check_verify(out, shreds, pubs, errmode)
        assert sv.stats() == (int((want != FD_SHRED_HIP_NO_ROOT).sum()), distinct)
        assert distinct < len(shreds) // 4
    finally:
        verifier.set_errmode(ERRMODE_AVX512)
        sv.close()


# ---- 5. handle reuse ----------------------------------------------------------------

def test_handle_reuse(verifier, golden):
    import torch
    shreds, pubs = verify_batch(golden)
    n_max = 96
    sv = ShredVerifier(verifier, n_max)
    try:
        a = (shreds[:n_max], pubs[:n_max])                 # n = n_max
        b = (shreds[n_max:n_max + 70], pubs[n_max:n_max + 70])
        out_a = launch_verify(sv, *a)
        out_b = launch_verify(sv, *b)                      # no sync between the two
        torch.cuda.synchronize()
        check_verify(out_a, *a, ERRMODE_AVX512)
        check_verify(out_b, *b, ERRMODE_AVX512)
        assert sv.stats()[1] == expected_codes(*b, ERRMODE_AVX512)[1]

        roots, flags, codes, keep = out_a
        with pytest.raises(ValueError):
            more = shreds[:n_max + 1]
            pool, off, sz = S.pack(more)
            big = [torch.full((m,), 0x5A, dtype=torch.uint8, device="cuda") for m in (32 * (n_max + 1), n_max + 1, n_max + 1)]
            try:
                sv.verify_dev(n_max + 1, _dev(pool), _dev(off), _dev(sz),
                              _dev(np.frombuffer(b"".join(pubs[:n_max + 1]), np.uint8)), big[0], big[1], big[2].view(torch.int8))
            finally:
                torch.cuda.synchronize()
                assert all(bool((t == 0x5A).all()) for t in big)   # untouched
        rc = replay.lib().fd_shred_hip_verify_dev(sv.s, 0, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                                                  keep[3].data_ptr(), roots.data_ptr(), flags.data_ptr(), codes.data_ptr(), None)
        assert rc == 0
        assert replay.lib().fd_shred_hip_verify_dev(sv.s, n_max + 1, keep[0].data_ptr(), keep[1].data_ptr(),
                                                    keep[2].data_ptr(), keep[3].data_ptr(), roots.data_ptr(),
                                                    flags.data_ptr(), codes.data_ptr(), None) == -1
        torch.cuda.synchronize()
        check_verify(out_a, *a, ERRMODE_AVX512)            # n = 0 and the refused call wrote nothing
    finally:
        sv.close()
