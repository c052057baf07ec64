"""bench.py's plain run and --dump-outputs: the arrays of the last timed step, exact in float32 / float64, within 64 MB,
the same on every run with the same arguments, and equal to what the oracle computes from the same stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _fake_step(C, cap, nblk, seed=1):
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, 256, (C, cap, 64), dtype=np.uint8)
    recs.view(oracle.REC_DTYPE)[..., 0]["variance"] = rng.standard_normal((C, cap)).astype(np.float32)
    counts = rng.integers(0, cap + 3, C).astype(np.int32)          # mode 0 counts events beyond rec_cap too
    nsyms = rng.integers(0, 194, (C, nblk)).astype(np.int32)
    syms = rng.standard_normal((C, nblk * 193 + 8)).astype(np.float32)
    return counts, recs, syms, nsyms


def test_dump_is_exact_and_keeps_valid_rows_only(tmp_path):
    C, cap, nblk = 40, 10, 4
    counts, recs, syms, nsyms = _fake_step(C, cap, nblk)
    nbytes = bench.dump_outputs(str(tmp_path), counts, recs, syms, nsyms)
    d = _load(tmp_path)
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert nbytes == sum(a.nbytes for a in d.values())
    np.testing.assert_array_equal(d["channels"], np.arange(C))
    np.testing.assert_array_equal(d["counts"], counts)
    rec = recs.view(oracle.REC_DTYPE)[..., 0]
    valid = np.arange(cap)[None, :] < np.minimum(counts, cap)[:, None]
    for f in ("type", "votes", "golay_errs", "frame_errors", "flags", "fn", "sym_pos", "block"):
        np.testing.assert_array_equal(d["rec_" + f], rec[f][valid])
    assert d["rec_variance"].tobytes() == rec["variance"][valid].tobytes()
    assert d["rec_data"].astype(np.uint32).astype("<u4").tobytes() == np.ascontiguousarray(rec["data"][valid]).tobytes()
    np.testing.assert_array_equal(d["nsyms"], nsyms)
    prefix = np.concatenate([syms[c, :nsyms[c].sum()] for c in range(C)])
    assert d["syms"].tobytes() == prefix.tobytes()


def test_dump_samples_channels_by_shape_within_the_budget(tmp_path):
    C, cap, nblk = 300, 34, 16
    counts, recs, syms, nsyms = _fake_step(C, cap, nblk, seed=2)
    budget = 1_000_000
    n1 = bench.dump_outputs(str(tmp_path / "a"), counts, recs, syms, nsyms, budget=budget)
    counts2, recs2, syms2, nsyms2 = _fake_step(C, cap, nblk, seed=3)          # other values, same shapes
    n2 = bench.dump_outputs(str(tmp_path / "b"), counts2, recs2, syms2, nsyms2, budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert n1 <= budget and n2 <= budget
    sel = a["channels"].astype(np.int64)
    assert 0 < len(sel) < C and np.all(np.diff(sel) > 0)
    np.testing.assert_array_equal(a["channels"], b["channels"])
    np.testing.assert_array_equal(a["counts"], counts[sel])
    # the default budget holds the headline's whole step: 16,384 channels x 34 record slots
    assert 16384 * (16 + 34 * 104) <= bench.DUMP_BUDGET < 64_000_000


@pytest.mark.gpu
def test_plain_bench_dumps_its_last_step_reproducibly(tmp_path):
    """A plain run measures the headline only; its dump is the same on two runs (their settle call counts differ) and
    equals the oracle's records for the last timed step of the same stream fed from a fresh state."""
    import m17_sdr_amd as m
    C, nblk, steps, warm = 64, 8, 3, 2
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "M17_BENCH_BACKEND"):
        env.pop(k, None)
    lines = []
    for k in range(2):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warm),
                            "--channels", str(C), "--blocks", str(nblk), "--dump-outputs", str(tmp_path / f"run{k}")],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    line = lines[0]
    assert line["steps"] == steps and line["roofline"]["calls_timed"] == steps and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None
    assert not {"noisy", "step_12_blocks", "two_contexts", "fir_stage", "fanout"} & set(line)
    a, b = _load(tmp_path / "run0"), _load(tmp_path / "run1")
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert a[name].tobytes() == b[name].tobytes(), name

    rx = m.Receiver(C, nblk)
    iq = rx.gen_batch(nblk * (warm + steps), n_stream_frames=40, ebn0_db=200.0)["iq"].cpu().numpy()
    rx.close()
    och = oracle.Channels(C)
    for k in range(warm + steps):
        ref = och.rx_blocks(np.ascontiguousarray(iq[:, k * nblk:(k + 1) * nblk]), mode=1, want_syms=False, nthreads=4)
    bench.dump_outputs(str(tmp_path / "oracle"), ref["counts"], ref["recs"].view(np.uint8).reshape(C, -1, 64))
    o = _load(tmp_path / "oracle")
    assert sorted(o) == sorted(a)
    for name in a:
        assert a[name].tobytes() == o[name].tobytes(), name
    assert a["counts"].sum() > 0 and ((a["rec_flags"].astype(np.int64) & m.F_DELIVERED) != 0).any()
