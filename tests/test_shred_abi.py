"""CPU: the shred-root entry points are exported, their header is plain C17, and
the Python wrappers check their tensors before any GPU call."""
import os
import re
import subprocess

import pytest

from firedancer_amd import replay
from firedancer_amd.build import LIB, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_shred_hip_new", "fd_shred_hip_delete", "fd_shred_hip_roots_dev", "fd_shred_hip_verify_dev",
       "fd_shred_hip_stats", "fd_sha256_hip_batch_dev")


def test_exports():
    build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(re.findall(r" T (\w+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= set(replay.EXPORTS)


def test_header_is_c17(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <sys/types.h>\n#include "fd_replay_hip.h"\n'
                   'static void * const fns[] = {\n' + "".join(f"  (void *){n},\n" for n in NEW) + '};\n'
                   'int main( void ) { return fns[0]==0 || FD_SHRED_HIP_NO_ROOT!=1; }\n')
    subprocess.check_call(["gcc", "-std=c17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


class _Tensor:
    """what ed25519._ptr reads of a GPU tensor; its address is never a real one"""
    is_cuda = True

    def __init__(self, nbytes, device=0):
        self._n = nbytes
        self.device = type("D", (), {"index": device})()

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def element_size(self):
        return 1

    def data_ptr(self):
        return 0x1000


class _Verifier:
    ctx, device = None, 0

    def _stream(self, stream):
        raise AssertionError("reached the GPU call")


def _args(n, short):
    sizes = {"pool": 1, "off": 4 * n, "sz": 4 * n, "pubs": 32 * n, "roots": 32 * n, "flags": n, "codes": n, "out": 32 * n}
    return {k: _Tensor(v - 1 if k == short else v) for k, v in sizes.items()}


@pytest.mark.parametrize("short", ["off", "sz", "roots", "flags"])
def test_roots_wrapper_rejects_short_tensors(short):
    a = _args(65, short)
    with pytest.raises(ValueError, match=short):
        replay.shred_roots_dev(_Verifier(), 65, a["pool"], a["off"], a["sz"], a["roots"], a["flags"])


@pytest.mark.parametrize("short", ["off", "sz", "pubs", "roots", "flags", "codes"])
def test_verify_wrapper_rejects_short_tensors(short):
    a = _args(65, short)
    sv = replay.ShredVerifier.__new__(replay.ShredVerifier)       # no handle: the checks come first
    sv.verifier, sv.s, sv.n_max, sv._lib = _Verifier(), None, 128, None
    with pytest.raises(ValueError, match=short):
        replay.shred_verify_dev(sv, 65, a["pool"], a["off"], a["sz"], a["pubs"], a["roots"], a["flags"], a["codes"])


@pytest.mark.parametrize("short", ["off", "sz", "out"])
def test_sha256_wrapper_rejects_short_tensors(short):
    a = _args(65, short)
    with pytest.raises(ValueError, match=short):
        replay.sha256_batch_dev(_Verifier(), 65, a["pool"], a["off"], a["sz"], a["out"])


def test_wrappers_reject_host_arrays():
    import numpy as np
    a = _args(4, None)
    with pytest.raises(TypeError):
        replay.shred_roots_dev(_Verifier(), 4, np.zeros(4096, np.uint8), a["off"], a["sz"], a["roots"], a["flags"])
