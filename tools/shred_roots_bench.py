#!/usr/bin/env python3
"""Times the shred-root path on the GPU (numbers for DESIGN.md, not a gate):

  fd_shred_hip_roots_dev   at 4096 and 65536 resident shreds (shreds/s)
  fd_shred_hip_verify_dev  on bursts of 64, 512 and 4096 shreds (latency of
                           one call, submit to synchronise)
  the comparator           tests/shred_lib.py's hashlib restatement on one
                           core of the same box (Python and OpenSSL; NOT the
                           reference's C, which this box does not have)

Input: FEC sets of 32 data + 32 code shreds with real Merkle trees of depth 6
(built here with hashlib) over random payloads, each set's root signed by its
own key on the GPU; bursts are whole sets, shuffled, packed at byte
granularity.  Before anything is timed every root is compared with the
restatement's and every code with 0.

    python tools/shred_roots_bench.py            one JSON line per leg
"""
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import shred_lib as S  # noqa: E402

DEPTH = 6


def make_set(rng, k):
    """64 shreds of one FEC set: unsigned (signature bytes zero), and the root"""
    typ_d, typ_c = (0x80, 0x40) if k % 2 == 0 else (0x90, 0x60)
    shreds = [bytearray(S.make_shred(rng, typ_d if i < 32 else typ_c, DEPTH, i, fec_set_idx=64 * k)) for i in range(64)]
    level = []
    for i, b in enumerate(shreds):
        P = (1139 if i < 32 else 1164) - 20 * DEPTH
        level.append(hashlib.sha256(S.LEAF_PREFIX + bytes(b[64:64 + P])).digest())
    proofs = [[] for _ in range(64)]
    for lv in range(DEPTH):
        for i in range(64):
            proofs[i].append(level[(i >> lv) ^ 1][:20])
        level = [hashlib.sha256(S.NODE_PREFIX + level[2 * j][:20] + level[2 * j + 1][:20]).digest()
                 for j in range(len(level) // 2)]
    for i, b in enumerate(shreds):
        M = len(b) - 20 * DEPTH
        b[M:] = b"".join(proofs[i])
        b[0:64] = bytes(64)
    return shreds, level[0]


def main():
    import torch
    from firedancer_amd import ShredVerifier, Verifier, replay
    assert torch.cuda.is_available(), "needs the GPU"
    rng = np.random.default_rng(606)
    nsets = 64
    v = Verifier(device=0, chunk_sigs=1 << 16)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731

    sets, roots = zip(*(make_set(rng, k) for k in range(nsets)))
    prvs = rng.integers(0, 256, (nsets, 32), dtype=np.uint8)
    d_pubs = torch.zeros((nsets, 32), dtype=torch.uint8, device="cuda")
    d_sigs = torch.zeros((nsets, 64), dtype=torch.uint8, device="cuda")
    rpool = np.frombuffer(b"".join(roots) + bytes(16), np.uint8)
    v.sign_dev(nsets, dev(prvs), dev(rpool), dev(np.arange(nsets, dtype=np.uint32) * 32),
               dev(np.full(nsets, 32, np.uint32)), d_pubs, d_sigs)
    torch.cuda.synchronize()
    pubs, sigs = d_pubs.cpu().numpy(), d_sigs.cpu().numpy()
    shreds, leaders = [], []
    for k in range(nsets):
        for b in sets[k]:
            b[0:64] = sigs[k].tobytes()
            shreds.append(bytes(b)); leaders.append(pubs[k].tobytes())
    want_roots = np.repeat(np.array([np.frombuffer(r, np.uint8) for r in roots]), 64, axis=0)

    def timed(fn, min_s=0.5):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); one = time.perf_counter() - t0
        reps = max(5, int(min_s / max(one, 1e-6)))
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, reps

    out = []
    # ---- roots, resident ----------------------------------------------------
    for n in (4096, 65536):
        order = np.concatenate([rng.permutation(4096) for _ in range(n // 4096)])
        pool, off, sz = S.pack([shreds[i] for i in order])
        d_pool, d_off, d_sz = dev(pool), dev(off), dev(sz)
        d_roots = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d_flags = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                         # the context's stream does not wait for torch's
        replay.shred_roots_dev(v, n, d_pool, d_off, d_sz, d_roots, d_flags, stream="ctx")
        v.sync()
        assert bool((d_flags == 1).all()) and np.array_equal(d_roots.cpu().numpy(), want_roots[order]), "roots differ"
        t, reps = timed(lambda: replay.shred_roots_dev(v, n, d_pool, d_off, d_sz, d_roots, d_flags, stream="ctx"))
        out.append({"leg": "roots_dev", "shreds": n, "ms_per_call": round(t * 1e3, 4), "shreds_per_s": round(n / t),
                    "hashed_GB_per_s": round(float(sz.sum()) / t / 1e9, 2), "reps": reps})
    # ---- verify bursts ------------------------------------------------------------
    sv = ShredVerifier(v, 4096)
    for n in (64, 512, 4096):
        order = rng.permutation(n)                       # n / 64 whole sets, shuffled
        pool, off, sz = S.pack([shreds[i] for i in order])
        d_pool, d_off, d_sz = dev(pool), dev(off), dev(sz)
        d_lead = dev(np.frombuffer(b"".join(leaders[i] for i in order), np.uint8))
        d_roots = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d_flags = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        d_codes = torch.full((n,), 0x5A, dtype=torch.int8, device="cuda")

        def call():
            sv.verify_dev(n, d_pool, d_off, d_sz, d_lead, d_roots, d_flags, d_codes, stream="ctx")
            v.sync()
        torch.cuda.synchronize()
        call()
        assert bool((d_codes == 0).all()) and np.array_equal(d_roots.cpu().numpy(), want_roots[order]), "verify differs"
        assert sv.stats() == (n, n // 64), sv.stats()
        for _ in range(10):
            call()
        lat = []
        for _ in range(200):
            t0 = time.perf_counter(); call(); lat.append(time.perf_counter() - t0)
        lat.sort()
        out.append({"leg": "verify_dev", "shreds": n, "distinct": n // 64, "us_median": round(statistics.median(lat) * 1e6, 1),
                    "us_p10": round(lat[20] * 1e6, 1), "us_p90": round(lat[180] * 1e6, 1),
                    "shreds_per_s_at_median": round(n / statistics.median(lat))})
    sv.close()
    # ---- one core, hashlib restatement ------------------------------------------------
    t0 = time.perf_counter()
    cpu = [S.shred_root(s) for s in shreds]
    t = time.perf_counter() - t0
    assert all(f == 1 and r == want_roots[i].tobytes() for i, (f, r) in enumerate(cpu))
    out.append({"leg": "cpu_hashlib_restatement_one_core", "shreds": len(shreds), "shreds_per_s": round(len(shreds) / t),
                "us_per_shred": round(t / len(shreds) * 1e6, 2)})
    for r in out:
        print(json.dumps(r))
    v.close()


if __name__ == "__main__":
    main()
