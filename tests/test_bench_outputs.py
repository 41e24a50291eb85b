"""bench.py's plain run and --dump-outputs.

CPU: dump_outputs over a made-up batch result -- the arrays' names, types
and contents (sizes, MD5 bytes, CRC-32 of every image, the seeded byte
sample), identical from call to call.
GPU: a small plain run really takes --steps timed steps, reports
ms_per_step, runs none of the --full legs, and two runs with the same
arguments dump the same arrays.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import bench

NAMES = {"image_sample", "track_image_crc32", "track_md5", "track_status", "track_out_offset",
         "track_bytes", "track_n_frames", "track_min_frame_bytes", "track_max_frame_bytes"}


def _load(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in os.listdir(d)}


def test_dump_outputs_arrays(tmp_path):
    from audiotools import _atgpu
    rng = np.random.RandomState(3)
    buf = rng.randint(0, 256, 5000).astype(np.uint8)
    res = []
    for off, n in ((0, 1234), (1240, 1), (2000, 3000)):  # gaps between the images
        r = _atgpu.TrackResult()
        r.out_offset, r.bytes, r.n_frames = off, n, 2
        r.min_frame_bytes, r.max_frame_bytes = 10, 20
        r.md5[:] = bytes(rng.randint(0, 256, 16).astype(np.uint8))
        res.append(r)
    out = torch.from_numpy(buf.copy())
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, out, res)
    bench.dump_outputs(b, out, res)
    da, db = _load(a), _load(b)
    assert set(da) == NAMES
    for k, v in da.items():
        assert v.dtype in (np.float32, np.float64) and np.array_equal(v, db[k]), k
    assert sum(v.nbytes for v in da.values()) <= 64 << 20
    assert da["track_bytes"].tolist() == [1234, 1, 3000]
    assert da["track_out_offset"].tolist() == [0, 1240, 2000]
    for t, r in enumerate(res):
        img = buf[r.out_offset:r.out_offset + r.bytes]
        assert da["track_image_crc32"][t] == zlib.crc32(img.tobytes())
        assert da["track_md5"][t].astype(np.uint8).tobytes() == bytes(r.md5)
        # every sampled value is a byte of this image
        assert set(da["image_sample"][t].astype(np.uint8)) <= set(img)
    assert np.all(da["image_sample"][1] == buf[1240])
    assert len(set(da["image_sample"][2])) > 200
    # a change of one sampled image shows
    buf2 = buf.copy()
    buf2[1240] ^= 0xFF
    c = str(tmp_path / "c")
    bench.dump_outputs(c, torch.from_numpy(buf2), res)
    dc = _load(c)
    assert not np.array_equal(dc["image_sample"], da["image_sample"])
    assert dc["track_image_crc32"][1] != da["track_image_crc32"][1]


def _plain(tmp, name, steps):
    d = os.path.join(tmp, name)
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--tracks", "5", "--frames", "3", "--dump-outputs", d],
                       capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), _load(d)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeat(tmp_path):
    line, da = _plain(str(tmp_path), "a", 3)
    assert line["metric"] == bench.METRIC and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same clock: 5 tracks x 3 frames per step
    # (ms_per_step is rounded to 1 us: under 1% of a step of 0.1 ms or more)
    assert line["value"] == pytest.approx(15 / (line["ms_per_step"] / 1e3), rel=1e-2)
    for leg in ("decode", "convert", "replaygain", "host_to_host", "resample", "chain",
                "replaygain_config4", "track2track", "narrow_batches", "plan_per_batch",
                "cpu_baseline", "verified_vs_oracle", "roofline", "roofline_valu"):
        assert leg not in line, leg
    assert set(da) == NAMES
    assert da["image_sample"].shape == (5, 8192) and da["image_sample"].dtype == np.float32
    assert np.all(da["track_status"] == 0) and np.all(da["track_n_frames"] == 3)
    line2, db = _plain(str(tmp_path), "b", 2)
    assert line2["steps"] == 2
    for k in da:
        assert np.array_equal(da[k], db[k]), k
