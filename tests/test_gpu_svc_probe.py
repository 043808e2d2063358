"""The verify service step by step (integration/svc_probe.c), on the GPU: a
segment in the probe's own memory, requests posted by hand through
include/fd_verify_svc.h's tile-side calls, each step under a deadline.

The service must take a frag request to INGESTED and RESULTS (every
zero-byte frag failing its parse, as fd_txn_parse fails it), retire a flush
of host-written entries, and tear down."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(REPO, "oracle", "_ref", "integration", "svc_probe")

pytestmark = pytest.mark.gpu


def test_probe_steps():
    if not os.path.exists(PROBE):
        pytest.skip("oracle/_ref/integration/svc_probe not built (build() with the reference sources)")
    r = subprocess.run(["timeout", "-k", "5", "40", PROBE, "64"], capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "PROBE OK" in out, out[-3000:]
    assert "64 frags, 64 parse failures" in out, out[-3000:]
    assert "latency: post -> INGESTED" in out, out[-3000:]
