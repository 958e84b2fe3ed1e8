"""Device time of a BPR epoch (irs_bpr_run_epochs) at a synthetic shape, ML-20M by default, for n_components = 64
and 128 and batch_size = 4096, 16384 and 65536: milliseconds per epoch by phase from ``irs_bpr_stats`` (sampler,
gradient, apply; HIP events round every launch, switched on here with ``IRSPACK_AMD_BPR_PHASES=1``), the epoch
without those events, and next to them two floors from bytes per triple:

- ``hbm_floor_ms``: every byte of a batch - three gathered rows per triple, the 8-byte words of the fixed-point sums,
  and the apply pass over the rows the batch touched (counted from the sampled batches) - at the device copy rate
  measured in ``profiles/`` (the newest ``r*_bench_line.json``);
- ``atomic_floor_ms``: the bytes of the integer atomics alone at 1.3 TB/s, the chip-wide rate measured for FLOAT
  atomic adds; the 64-bit integer form is assumed, not measured, to run at the same byte rate.

One JSON line per point.  Run it under a time limit sized to the step, e.g.

    timeout -k 10 420 python scripts/bpr_bench.py
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["IRSPACK_AMD_BPR_PHASES"] = "1"  # (read when a handle is made)

from irspack_amd.recommenders.bpr import BPRFMTrainer  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402

ATOMIC_GBS = 1300.0


def measured_copy_gbs() -> float:
    lines = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_line.json")))
    for path in reversed(lines):
        try:
            found = json.load(open(path)).get("ceilings", {}).get("copy_gbs") or json.load(open(path)).get("copy_gbs")
        except (OSError, ValueError, AttributeError):
            found = None
        if found:
            return float(found)
    raise SystemExit("no measured copy rate under profiles/")


def touched_rows_per_triple(trainer: BPRFMTrainer, batch: int, n_batches: int = 8) -> float:
    """distinct user rows + distinct item rows per triple, over the first batches of epoch 0"""
    n = trainer.epoch_length
    rows = triples = 0
    for first in range(0, min(n, batch * n_batches), batch):
        u, i, j = trainer.sample(0, first, min(batch, n - first))
        rows += np.unique(u).size + np.unique(np.concatenate([i, j])).size
        triples += u.size
    return rows / max(triples, 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--k", default="64,128")
    ap.add_argument("--batch", default="4096,16384,65536")
    ap.add_argument("--epochs", type=int, default=2)
    args = ap.parse_args()
    X = make_interactions(args.shape).astype(np.float32)
    copy_gbs = measured_copy_gbs()
    warm = BPRFMTrainer(X[:2000], 8, 1e-9, 1e-9, batch_size=256)
    warm.run_epochs(1)  # (the first call of a process pays the code-object load)
    warm.close()
    for k in (int(v) for v in args.k.split(",")):
        for batch in (int(v) for v in args.batch.split(",")):
            os.environ["IRSPACK_AMD_BPR_PHASES"] = "0"
            plain = BPRFMTrainer(X, k, 1e-9, 1e-9, batch_size=batch)
            plain.run_epochs(1)
            t0 = time.perf_counter()
            plain.run_epochs(args.epochs)
            wall = (time.perf_counter() - t0) / args.epochs
            epoch_ms = plain.stats()["epoch_ms"]
            plain.close()
            os.environ["IRSPACK_AMD_BPR_PHASES"] = "1"
            timed = BPRFMTrainer(X, k, 1e-9, 1e-9, batch_size=batch)
            timed.run_epochs(2)
            st = timed.stats()
            kp = (k + 3) // 4 * 4
            n = timed.epoch_length
            touched = touched_rows_per_triple(timed, batch)
            timed.close()
            gather = 3 * kp * 4 + 12
            atomics = (3 * kp + 2) * 8
            apply_bytes = touched * kp * 32  # theta, G and the 8-byte sum read, then all three written
            per_triple = gather + atomics + apply_bytes
            out = dict(shape=args.shape, n_users=X.shape[0], n_items=X.shape[1], n_triples=n, k=k, batch_size=batch,
                       batches_per_epoch=st["batches_per_epoch"], lanes_per_triple=st["lanes_per_triple"],
                       scale_log2=st["scale_log2"], epoch_ms=round(epoch_ms, 2), wall_ms_per_epoch=round(wall * 1e3, 2),
                       epoch_ms_with_phase_events=round(st["epoch_ms"], 2), sample_ms=round(st["sample_ms"], 2),
                       grad_ms=round(st["grad_ms"], 2), apply_ms=round(st["apply_ms"], 2),
                       touched_rows_per_triple=round(touched, 4), bytes_per_triple=round(per_triple, 1),
                       copy_gbs=round(copy_gbs, 1), hbm_floor_ms=round(n * per_triple / copy_gbs / 1e6, 2),
                       atomic_floor_ms=round(n * atomics / ATOMIC_GBS / 1e6, 2))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
