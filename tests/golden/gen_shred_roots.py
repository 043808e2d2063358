#!/usr/bin/env python3
"""Regenerates tests/golden/shred_roots.npz: shreds and the reference's Merkle
root of each (fd_shred_parse + fd_shred_merkle_root through
tests/golden/shred_roots_drv.c).

    python tests/golden/gen_shred_roots.py [REF]      (REF: the reference checkout, default /root/reference)

The driver is compiled with the reference's sources where they lie, with the
flags and the object list of integration/Makefile's fec target, into a
temporary directory; nothing of it is kept.  Contents of the .npz:
tests/shred_lib.py load_golden.

(a) synthetic shreds (tests/shred_lib.py make_shred, seed fixed): the six
    Merkle types x proof depths 0..9, each with the lowest tree index of its
    type, the highest (2^d - 1, capped by the in-type bound of 67 per type)
    and one between.  A code shred's tree index is code.idx + data_cnt >= 1,
    so the three code types have no valid shred at depth 0.
(b) two FEC sets of the reference's shredder, 32 data + 32 code each.
"""
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import shred_lib as S  # noqa: E402

FLAGS = ("-O3 -fPIC -std=c17 -D_GNU_SOURCE -ffunction-sections -fdata-sections -DFD_HAS_HOSTED=1 -DFD_HAS_INT128=1 "
         "-DFD_HAS_DOUBLE=1 -DFD_HAS_ALLOCA=1 -DFD_HAS_X86=1 -DFD_HAS_ATOMIC=1 -DFD_HAS_THREADS=1 -march=x86-64 "
         "-mtune=generic -w").split()
# integration/Makefile: SRCS, FEC_SRCS and the ed25519 part of RPL_SRCS
SRCS = ("tango/dcache/fd_dcache.c tango/mcache/fd_mcache.c tango/tcache/fd_tcache.c tango/fseq/fd_fseq.c "
        "tango/tempo/fd_tempo.c util/math/fd_stat.c util/rng/fd_rng_secure.c disco/topo/fd_topo.c disco/topo/fd_topob.c "
        "disco/metrics/fd_metrics.c util/pod/fd_pod.c ballet/txn/fd_txn_parse.c util/fd_hash.c util/fd_util.c "
        "util/log/fd_log.c util/log/fd_backtrace.c util/tile/fd_tile.c util/cstr/fd_cstr.c util/io/fd_io.c "
        "util/env/fd_env.c ballet/sha512/fd_sha512.c ballet/hex/fd_hex.c "
        "disco/shred/fd_shredder.c ballet/shred/fd_shred.c ballet/bmtree/fd_bmtree.c ballet/sha256/fd_sha256.c "
        "ballet/reedsol/fd_reedsol.c ballet/reedsol/fd_reedsol_pi.c "
        "ballet/ed25519/fd_ed25519_user.c ballet/ed25519/fd_curve25519.c ballet/ed25519/fd_curve25519_scalar.c "
        "ballet/ed25519/fd_f25519.c").split()
SRCS += [f"ballet/reedsol/fd_reedsol_encode_{n}.c" for n in (16, 32, 64, 128)]
SRCS += [f"ballet/reedsol/fd_reedsol_recover_{n}.c" for n in (16, 32, 64, 128, 256)]
SRCS += [f"ballet/reedsol/wrapped_impl/fd_reedsol_ppt_impl_{n}.c" for n in (17, 25, 33, 40, 45, 50, 55, 60, 65)]
SRCS += [f"ballet/reedsol/wrapped_impl/fd_reedsol_fft_impl_{n}.c" for n in ("128_0", "128_128", "256_0", "64_0", "64_128",
                                                                             "64_64")]


def build_driver(ref, tmp):
    def cc(src):
        obj = os.path.join(tmp, src.replace("/", "_")[:-2] + ".o")
        # cwd: fd_reedsol.c imports its constant tables by a path relative to the reference's root
        subprocess.check_call(["gcc", *FLAGS, "-c", os.path.join(ref, "src", src), "-o", obj], cwd=ref)
        return obj
    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(cc, SRCS))
    exe = os.path.join(tmp, "shred_roots_drv")
    subprocess.check_call(["gcc", *FLAGS, "-I" + os.path.join(ref, "src", "disco", "shred"), "-o", exe,
                           os.path.join(HERE, "shred_roots_drv.c"), *objs, "-Wl,--gc-sections", "-lpthread", "-lm"])
    return exe


def synthetic(rng):
    out, meta = [], []
    for typ in S.MERKLE_TYPES:
        data = typ in S.DATA_TYPES
        for d in range(S.DEPTH_MAX + 1):
            lo = 0 if data else 1
            hi = min((1 << d) - 1, S.IN_TYPE_MAX - 1 if data else 2 * S.IN_TYPE_MAX - 1)
            if hi < lo:
                continue                                   # code, depth 0
            for t in sorted({lo, hi, (lo + hi + 1) // 2}):
                data_cnt = min(S.IN_TYPE_MAX, t)
                out.append(S.make_shred(rng, typ, d, t, data_cnt=data_cnt, code_cnt=S.IN_TYPE_MAX))
                meta.append((typ, d, t))
    return out, meta


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    shreds, meta = synthetic(np.random.default_rng(20250607))
    n = len(shreds)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref, tmp)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", n))
            for s in shreds:
                f.write(struct.pack("<I", len(s)) + s.ljust(S.MAX_SZ, b"\0"))
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    syn_out = np.frombuffer(raw[:33 * n], np.uint8).reshape(n, 33)
    assert syn_out[:, 0].all(), ("the reference rejected synthetic shreds", [meta[i] for i in np.nonzero(syn_out[:, 0] == 0)[0]])
    leader = np.frombuffer(raw[33 * n:33 * n + 32], np.uint8)
    rec = np.dtype([("sz", "<u4"), ("shred", "u1", (S.MAX_SZ,)), ("ok", "u1"), ("root", "u1", (32,))])
    sets = np.frombuffer(raw[33 * n + 32:], rec).reshape(2, 64)
    assert sets["ok"].all()
    syn = np.zeros((n, S.MAX_SZ), np.uint8)
    for i, s in enumerate(shreds):
        syn[i, :len(s)] = np.frombuffer(s, np.uint8)
    path = os.path.join(HERE, "shred_roots.npz")
    np.savez_compressed(path, syn=syn, syn_sz=np.array([len(s) for s in shreds], np.uint32),
                        syn_root=syn_out[:, 1:].copy(), set=sets["shred"].copy(), set_sz=sets["sz"].copy(),
                        set_root=sets["root"].copy(), leader=leader.copy())
    print(f"{path}: {n} synthetic + 128 shredder shreds, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
