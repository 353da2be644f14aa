"""A plain bench.py run and its --dump-outputs: the line carries the headline
alone (what --full adds is absent), --steps sets the timed steps, and the
dumped arrays are the last timed step's outputs -- float32, every frame's
status 0, the flags of the batch, and a wire that the oracle reproduces
byte for byte from the dumped payload at the nonces the send counter must
have reached (DUMP_NONCE, one untimed pass, then the timed steps), which is
also what makes two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P, K = 512, 1024, 2


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(K), "--warmup", "1", "--msgs", str(N),
                        "--dump-outputs", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_plain_line_is_the_headline_alone(plain_run):
    d, _ = plain_run
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == K and d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    # value and ms_per_step say the same thing: K steps of N x P payload bytes
    assert d["value"] == pytest.approx(N * P / 2**30 / (d["ms_per_step"] / 1e3), rel=1e-9)
    for k in ("roofline", "hbm_fed", "configs", "host_paths", "cpu_baseline", "eager_ms_per_step"):
        assert k not in d, k


def test_dump_is_the_last_timed_step(plain_run):
    import torch

    import bench
    from libzmq_amd import curve as C
    from oracle import oracle as O

    _, a = plain_run
    assert sorted(a) == ["flags", "payload", "sampled_frames", "status", "wire"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    W = C.wire_size(0, 0, P)
    frames = a["sampled_frames"].astype(np.int64)
    m = len(frames)
    assert m == min(N, bench.DUMP_ELEMS // W) and (np.diff(frames) > 0).all() and frames[-1] < N
    assert a["wire"].shape == (m, W) and a["payload"].shape == (m, P)
    assert (a["status"] == 0).all()
    flags = np.where(frames % 16 == 15, 1, 0).astype(np.uint8)
    assert np.array_equal(a["flags"], flags)
    wire = a["wire"].astype(np.uint8)
    assert np.array_equal(wire, a["wire"])  # bytes, exactly
    payload = a["payload"].astype(np.uint8)
    # the send counter: DUMP_NONCE, one untimed pass of K steps, K - 1 timed steps before the last
    nonce = (bench.DUMP_NONCE + (2 * K - 1) * N + frames).astype(np.uint64)
    assert np.array_equal(wire[:, 8:16], nonce.astype(">u8").view(np.uint8).reshape(m, 8))
    precom = bytes(torch.randint(0, 256, (32,), dtype=torch.uint8,
                                 generator=torch.Generator().manual_seed(0x5EED)).tolist())
    in_off = np.arange(m, dtype=np.uint64) * P
    out_off = np.arange(m, dtype=np.uint64) * W
    ref = O.encode_batch(O.make_sessions([precom]), np.zeros(m, np.uint32), nonce, flags, in_off,
                         np.full(m, P, np.uint32), np.concatenate([payload.ravel(), np.zeros(1, np.uint8)]), out_off,
                         m * W)
    assert np.array_equal(wire.ravel(), ref)
