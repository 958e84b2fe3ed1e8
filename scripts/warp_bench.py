"""Device time of a WARP epoch (``BPRFMTrainer(loss="warp")``, DESIGN.md section 14, "WARP") at a synthetic shape,
ML-20M by default, for n_components = 64 and 128, batch_size = 4096, 16384 and 65536 and max_sampled = 10: for the
first epoch and for a later one (the 10th by default, where the search has grown longer) milliseconds per epoch, by
phase (search-and-gradient, apply; HIP events round every launch, ``IRSPACK_AMD_BPR_PHASES=1``), the mean number of
candidates examined and the share of positions without a violation; the same epochs with 1, 2 and 4 candidate rows
in flight (``IRSPACK_AMD_WARP_IN_FLIGHT``); the BPR epoch of the same shape measured in the same run; and two floors
from bytes (section 14's table):

- ``gather_floor_ms``: ``(2 + mean tries) * 4 kp`` bytes per position at the device copy rate measured in
  ``profiles/`` (the newest ``r*_bench_line.json``);
- ``atomic_floor_ms``: ``(3 kp + 2) * 8`` bytes per update at 1.3 TB/s, the chip-wide rate measured for FLOAT atomic
  adds (assumed for the 64-bit integer form).

One JSON line per point.  Run it under a time limit sized to the step, e.g.

    timeout -k 10 540 python scripts/warp_bench.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bpr_bench import ATOMIC_GBS, measured_copy_gbs  # noqa: E402
from irspack_amd.recommenders.bpr import BPRFMTrainer  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402


def trainer(X, k, batch, loss, phases, max_sampled, in_flight=None):
    os.environ["IRSPACK_AMD_BPR_PHASES"] = "1" if phases else "0"  # (both read when a handle is made)
    if in_flight is None:
        os.environ.pop("IRSPACK_AMD_WARP_IN_FLIGHT", None)
    else:
        os.environ["IRSPACK_AMD_WARP_IN_FLIGHT"] = str(in_flight)
    return BPRFMTrainer(X, k, 1e-9, 1e-9, loss=loss, batch_size=batch, max_sampled=max_sampled)


def warp_epochs(t, later):
    """stats of epoch 1 and of epoch ``later`` of a fresh trainer"""
    out = []
    for n in (1, later - 1):
        if n > 1:
            t.run_epochs(n - 1)
        t.run_epochs(1)
        out.append(t.warp_stats())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--k", default="64,128")
    ap.add_argument("--batch", default="4096,16384,65536")
    ap.add_argument("--max-sampled", type=int, default=10)
    ap.add_argument("--later-epoch", type=int, default=10)
    ap.add_argument("--in-flight", default="1,2,4")
    args = ap.parse_args()
    X = make_interactions(args.shape).astype(np.float32)
    copy_gbs = measured_copy_gbs()
    for loss in ("bpr", "warp"):  # (the first call of a process pays the code-object load)
        warm = trainer(X[:2000], 8, 256, loss, False, args.max_sampled)
        warm.run_epochs(1)
        warm.close()
    for k in (int(v) for v in args.k.split(",")):
        kp = (k + 3) // 4 * 4
        for batch in (int(v) for v in args.batch.split(",")):
            point = dict(shape=args.shape, n_users=X.shape[0], n_items=X.shape[1], k=k, batch_size=batch,
                         max_sampled=args.max_sampled, later_epoch=args.later_epoch)
            try:
                bpr = trainer(X, k, batch, "bpr", False, args.max_sampled)
                bpr.run_epochs(2)
                point.update(n_positions=bpr.epoch_length, bpr_epoch_ms=round(bpr.stats()["epoch_ms"], 2))
                bpr.close()
                bpr = trainer(X, k, batch, "bpr", True, args.max_sampled)
                bpr.run_epochs(2)
                st = bpr.stats()
                point.update(bpr_sample_ms=round(st["sample_ms"], 2), bpr_grad_ms=round(st["grad_ms"], 2),
                             bpr_apply_ms=round(st["apply_ms"], 2))
                bpr.close()
                for in_flight in (int(v) for v in args.in_flight.split(",")):
                    t = trainer(X, k, batch, "warp", False, args.max_sampled, in_flight)
                    first, later = warp_epochs(t, args.later_epoch)
                    t.close()
                    point[f"warp_epoch_ms_in_flight_{in_flight}"] = [round(first["epoch_ms"], 2), round(later["epoch_ms"], 2)]
                t = trainer(X, k, batch, "warp", False, args.max_sampled)
                stats = warp_epochs(t, args.later_epoch)
                t.close()
                t = trainer(X, k, batch, "warp", True, args.max_sampled)
                timed = warp_epochs(t, args.later_epoch)
                t.close()
                for name, st, ph in zip(("first", "later"), stats, timed):
                    n, tries = st["epoch_positions"], st["epoch_tries"] / max(st["epoch_positions"], 1)
                    gather = n * (2 + tries) * 4 * kp / copy_gbs / 1e6
                    atomic = st["epoch_updates"] * (3 * kp + 2) * 8 / ATOMIC_GBS / 1e6
                    point[name] = dict(
                        in_flight=st["in_flight"], epoch_ms=round(st["epoch_ms"], 2),
                        epoch_ms_with_phase_events=round(ph["epoch_ms"], 2), search_ms=round(ph["search_ms"], 2),
                        apply_ms=round(ph["apply_ms"], 2), mean_tries=round(tries, 4),
                        share_without_violation=round(1 - st["epoch_updates"] / max(n, 1), 4),
                        gather_floor_ms=round(gather, 2), atomic_floor_ms=round(atomic, 2),
                        floor_fraction=round((gather + atomic) / st["epoch_ms"], 4),
                        search_floor_fraction=round((gather + atomic) / max(ph["search_ms"], 1e-9), 4))
                point["scale_log2"] = stats[0]["scale_log2"]
            except RuntimeError as e:  # (a diverged fit: the synchronous step at a large batch, section 14)
                point["error"] = str(e)
            print(json.dumps(point), flush=True)


if __name__ == "__main__":
    main()
