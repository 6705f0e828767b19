"""GPU suite: bench.py's plain run, --dump-outputs and --full on a 2 % products-shaped graph."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale", "0.02", "--steps", "2", "--warmup", "1"]


def _bench(*extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(BASE + list(extra), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_dumps_identical_outputs_and_full_adds_the_other_legs(tmp_path):
    """Two plain runs with --dump-outputs (default dropout 0.5: seeded masks) write the same arrays, bit for bit: the loss (float64),
    the training rows' log-probabilities and every parameter's gradient and post-step value (float32), < 64 MB in all.  The plain
    line carries the headline keys and none of the --full legs; --full adds them and times the same headline steps."""
    lines, dumps = [], []
    for i in range(2):
        d = str(tmp_path / ("dump%d" % i))
        lines.append(_bench("--dump-outputs", d))
        dumps.append(_load(d))
    one, (a, b) = lines[0], dumps
    for key, kind in (("metric", str), ("value", float), ("unit", str), ("higher_is_better", bool), ("dtype", str), ("ms_per_step", float)):
        assert isinstance(one[key], kind), key
    assert one["steps"] == 2 and one["warmup"] == 1 and one["ms_per_step"] > 0 and one["value"] > 0
    for key in ("secondary", "epoch_ms_plain_model", "epoch_ms_last_layer_backward_on_loss_rows", "value_reference_modules"):
        assert key not in one, key
    assert one["cpu_baseline"] is None and one["roofline"]["traffic"] is None and "controls" not in one["roofline"]
    assert "predicted" not in one["config"]["partition"]

    assert sorted(a) == sorted(b)
    params = sorted(k[len("param."):] for k in a if k.startswith("param."))
    assert params and sorted(k[len("grad."):] for k in a if k.startswith("grad.")) == params
    assert set(a) == {"loss", "log_probs_train_rows"} | {"param." + p for p in params} | {"grad." + p for p in params}
    assert a["loss"].dtype == np.float64 and a["loss"].shape == (1,)
    assert all(v.dtype == np.float32 for k, v in a.items() if k != "loss")
    assert sum(v.nbytes for v in a.values()) < 64 << 20
    lp = a["log_probs_train_rows"]
    assert lp.ndim == 2 and lp.shape[0] > 0 and lp.shape[1] == 47
    assert np.allclose(np.exp(lp.astype(np.float64)).sum(1), 1.0, atol=1e-4)   # log-probabilities: every row sums to one
    assert a["loss"][0] == one["config"]["final_loss"]                          # the dump is the last timed step's loss
    for k in a:
        assert np.array_equal(a[k], b[k]), k

    full = _bench("--full", "--no-pmc", "--no-scale-model")
    assert full["epoch_ms_plain_model"] > 0 and full["epoch_ms_last_layer_backward_on_loss_rows"] > 0
    assert full["cpu_baseline"] is not None and full["cpu_baseline"]["value"] > 0
    assert "controls" in full["roofline"]
    # the headline steps come first and are the same computation with or without --full
    assert abs(full["config"]["final_loss"] - one["config"]["final_loss"]) <= 1e-6 * max(1.0, abs(one["config"]["final_loss"]))
