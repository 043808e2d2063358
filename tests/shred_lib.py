"""The shred Merkle root and its flag, restated in Python with hashlib, and a
builder of synthetic shreds (tests/test_shred_roots_ref.py checks the
restatement against the reference's roots in tests/golden/shred_roots.npz; the
GPU tests use it for inputs the fixture does not hold).

Definition (include/fd_replay_hip.h, shred section; the reference:
fd_shred_merkle_root, src/ballet/shred/fd_shred.c:108-131, with the bounds of
fec_hip_root in integration/fd_fec_resolver_hip.patch)."""
import hashlib
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shred_roots.npz")

LEAF_PREFIX = b"\x00SOLANA_MERKLE_SHREDS_LEAF"
NODE_PREFIX = b"\x01SOLANA_MERKLE_SHREDS_NODE"
assert len(LEAF_PREFIX) == 26 and len(NODE_PREFIX) == 26

MIN_SZ, MAX_SZ = 1203, 1228
MERKLE_TYPES = (0x80, 0x90, 0xB0, 0x40, 0x60, 0x70)   # data, chained, chained resigned; code likewise
DATA_TYPES = (0x80, 0x90, 0xB0)
RESIGNED = (0xB0, 0x70)
IN_TYPE_MAX = 67
DEPTH_MAX = 9

OFF_VARIANT, OFF_SLOT, OFF_IDX, OFF_VERSION, OFF_FEC_SET_IDX = 0x40, 0x41, 0x49, 0x4d, 0x4f
OFF_PARENT_OFF, OFF_FLAGS, OFF_SIZE = 0x53, 0x55, 0x56           # data
OFF_DATA_CNT, OFF_CODE_CNT, OFF_CODE_IDX = 0x53, 0x55, 0x57      # code


def shred_root(shred):
    """(flag, root): flag 1 and the 32-byte root, or 0 and 32 zero bytes.
    shred: bytes of exactly the size handed to the engine."""
    b = bytes(shred)
    sz = len(b)
    none = (0, bytes(32))
    if sz < MIN_SZ:
        return none
    variant = b[OFF_VARIANT]
    typ, d = variant & 0xf0, variant & 0x0f
    if typ not in MERKLE_TYPES or d > DEPTH_MAX:
        return none
    data = (typ & 0xC0) == 0x80
    r = 1 if typ in RESIGNED else 0
    S = MIN_SZ if data else MAX_SZ
    if sz < S:
        return none
    if data:
        idx, = struct.unpack_from("<I", b, OFF_IDX)
        fec, = struct.unpack_from("<I", b, OFF_FEC_SET_IDX)
        in_idx = (idx - fec) & 0xffffffff
        shred_idx = in_idx
    else:
        data_cnt, code_cnt, in_idx = struct.unpack_from("<HHH", b, OFF_DATA_CNT)
        if not (1 <= data_cnt <= IN_TYPE_MAX and 1 <= code_cnt <= IN_TYPE_MAX):
            return none
        shred_idx = in_idx + data_cnt
    if in_idx >= IN_TYPE_MAX or shred_idx >= (1 << d):
        return none
    P = (1139 if data else 1164) - 20 * d - 64 * r
    M = S - 20 * d - 64 * r
    assert M == 64 + P
    node = hashlib.sha256(LEAF_PREFIX + b[64:64 + P]).digest()
    for k in range(d):
        sib = b[M + 20 * k:M + 20 * k + 20]
        pair = node[:20] + sib if not (shred_idx >> k) & 1 else sib + node[:20]
        node = hashlib.sha256(NODE_PREFIX + pair).digest()
    return 1, node


def shred_roots(pool, off, sz):
    """flags (uint8[n]) and roots (uint8[n,32]) of shreds pool[off[i], +sz[i])."""
    n = len(off)
    flags, roots = np.zeros(n, np.uint8), np.zeros((n, 32), np.uint8)
    pb = bytes(np.asarray(pool, np.uint8))
    for i in range(n):
        f, r = shred_root(pb[int(off[i]):int(off[i]) + int(sz[i])])
        flags[i] = f
        roots[i] = np.frombuffer(r, np.uint8)
    return flags, roots


def make_shred(rng, typ, depth, shred_idx=0, sz=None, data_cnt=32, code_cnt=32, fec_set_idx=64, variant=None,
               idx=None, code_idx=None):
    """A synthetic shred of random bytes with the header fields that the root
    and fd_shred_parse read.  typ: one of the six Merkle types (or any high
    nibble, for rejects); shred_idx: the tree index (data: idx - fec_set_idx;
    code: code.idx + data_cnt).  variant / idx / code_idx override what
    typ, depth and shred_idx give.  Valid arguments give a shred that
    fd_shred_parse accepts."""
    data = (typ & 0xC0) == 0x80
    if sz is None:
        sz = MIN_SZ if data else MAX_SZ
    b = bytearray(rng.integers(0, 256, max(sz, MAX_SZ), dtype=np.uint8).tobytes())
    b[OFF_VARIANT] = (typ | depth) if variant is None else variant
    struct.pack_into("<Q", b, OFF_SLOT, 10)
    struct.pack_into("<H", b, OFF_VERSION, 6051)
    struct.pack_into("<I", b, OFF_FEC_SET_IDX, fec_set_idx)
    if data:
        struct.pack_into("<I", b, OFF_IDX, ((fec_set_idx + shred_idx) if idx is None else idx) & 0xffffffff)
        struct.pack_into("<H", b, OFF_PARENT_OFF, 1)
        b[OFF_FLAGS] = 0x00
        struct.pack_into("<H", b, OFF_SIZE, 0x58 + 200)           # header + 200 payload bytes
    else:
        ci = (shred_idx - data_cnt) if code_idx is None else code_idx
        struct.pack_into("<HHH", b, OFF_DATA_CNT, data_cnt, code_cnt, ci & 0xffff)
        struct.pack_into("<I", b, OFF_IDX, (fec_set_idx + max(ci, 0)) if idx is None else idx)
    return bytes(b[:sz])


def reject_cases(rng):
    """(name, shred bytes, expected flag): every reject class, and every
    condition at its last accepted value"""
    mk = lambda *a, **k: make_shred(rng, *a, **k)  # noqa: E731
    return [
        ("data sz 1202", mk(0x80, 3, 5, sz=1202), 0),
        ("data sz 1203", mk(0x80, 3, 5, sz=1203), 1),
        ("code sz 1227", mk(0x40, 7, 40, sz=1227), 0),
        ("code sz 1228", mk(0x40, 7, 40, sz=1228), 1),
        ("data sz 1228 (extra bytes)", mk(0x90, 3, 5, sz=1228), 1),
        ("legacy data 0xA5", mk(0x80, 5, 0, variant=0xA5), 0),
        ("legacy code 0x5A", mk(0x40, 10, 40, variant=0x5A, sz=1228), 0),
        ("unknown type 0xC0", mk(0x80, 6, 0, variant=0xC6), 0),
        ("unknown type 0x00", mk(0x80, 6, 0, variant=0x06), 0),
        ("d 10", mk(0x80, 10, 5), 0),
        ("d 9", mk(0x80, 9, 5), 1),
        ("data_cnt 0", mk(0x40, 7, 5, data_cnt=0, code_idx=5), 0),
        ("data_cnt 1", mk(0x40, 7, 6, data_cnt=1, code_idx=5), 1),
        ("data_cnt 67", mk(0x40, 8, 72, data_cnt=67, code_idx=5), 1),
        ("data_cnt 68", mk(0x40, 8, 73, data_cnt=68, code_idx=5), 0),
        ("code_cnt 0", mk(0x60, 7, 40, code_cnt=0), 0),
        ("code_cnt 1", mk(0x60, 7, 32, code_cnt=1), 1),
        ("code_cnt 67", mk(0x60, 7, 40, code_cnt=67), 1),
        ("code_cnt 68", mk(0x60, 7, 40, code_cnt=68), 0),
        ("data in-type index 66", mk(0xB0, 7, 66), 1),
        ("data in-type index 67", mk(0xB0, 7, 67), 0),
        ("code in-type index 66", mk(0x70, 8, 32 + 66, code_cnt=67), 1),
        ("code in-type index 67", mk(0x70, 8, 32 + 67, code_cnt=67), 0),
        ("idx < fec_set_idx", mk(0x80, 9, 0, idx=63, fec_set_idx=64), 0),
        ("shred_idx 2^d", mk(0x80, 4, 16), 0),
        ("shred_idx 2^d - 1", mk(0x80, 4, 15), 1),
        ("code shred_idx 2^d", mk(0x40, 6, 64), 0),
        ("code shred_idx 2^d - 1", mk(0x40, 6, 63), 1),
        ("data d 0", mk(0x80, 0, 0), 1),
        ("code d 0", mk(0x40, 0, 1, data_cnt=1), 0),
    ]


def pack(shreds, gaps=True):
    """Shreds back to back at byte granularity, a 1..15-byte gap cycling
    between them when gaps, 16 readable bytes after the last: (pool uint8,
    off uint32, sz uint32)."""
    off, parts, o = [], [], 0
    for i, s in enumerate(shreds):
        g = (1 + i % 15) if gaps else 0
        parts.append(bytes([0xA5] * g)); o += g
        off.append(o); parts.append(bytes(s)); o += len(s)
    parts.append(bytes(32))
    return (np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint32),
            np.array([len(s) for s in shreds], np.uint32))


def load_golden():
    """tests/golden/shred_roots.npz (tests/golden/gen_shred_roots.py): a dict with
      syn        uint8[n,1228]  synthetic shreds (data shreds use the first 1203 bytes)
      syn_sz     uint32[n]
      syn_root   uint8[n,32]    fd_shred_merkle_root of each
      set        uint8[2,64,1228]  two FEC sets of the reference's shredder, 32 data then 32 code
      set_sz     uint32[2,64]
      set_root   uint8[2,64,32]
      leader     uint8[32]      the key that signed both sets"""
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def golden_shreds(g):
    """every fixture shred as bytes of its own size, synthetic first, and their reference roots"""
    out = [bytes(g["syn"][i][:int(g["syn_sz"][i])]) for i in range(len(g["syn_sz"]))]
    roots = [g["syn_root"]]
    for s in range(g["set"].shape[0]):
        out += [bytes(g["set"][s, j][:int(g["set_sz"][s, j])]) for j in range(g["set"].shape[1])]
        roots.append(g["set_root"][s])
    return out, np.concatenate(roots)
