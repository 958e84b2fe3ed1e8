"""Device time of a Mult-VAE epoch (irs_multvae_run_epochs) at a synthetic shape, ML-20M by default, with the
constructor defaults of ``MultVAERecommender`` (dim_z 16, hidden 256, minibatch 512): milliseconds per epoch by phase
from ``irs_multvae_stats`` (HIP events round every phase, switched on here with ``IRSPACK_AMD_MULTVAE_PHASES=1``), the
epoch without those events, and next to them:

- the TFLOP/s of the three large products (logits, d[W4; b4], dh2: 2 U I (Hd + 1) flops each per epoch) against the
  fp32-MFMA ceiling the library measures on this device (``irs_measure_ceilings``);
- ``floor_ms``: those flops at that ceiling plus the bytes of the integer atomics of dW1 at 1.3 TB/s, the
  chip-wide rate measured for float atomic adds.

One JSON line.  Run it under a time limit sized to the step, e.g.

    timeout -k 10 300 python scripts/multvae_bench.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irspack_amd import _lib  # noqa: E402
from irspack_amd.recommenders.multvae import MultVAETrainer  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402

ATOMIC_GBS = 1300.0


def trainer_of(X, args) -> MultVAETrainer:
    return MultVAETrainer(X, args.dim_z, args.hidden, None, 0.5, 0.0, 0.2, 50, args.minibatch, 1e-3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--dim-z", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--minibatch", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    args = ap.parse_args()
    X = make_interactions(args.shape).astype(np.float32)
    U, I = X.shape
    ceiling = _lib.measure_ceilings()["mfma_f32_tflops"]
    os.environ["IRSPACK_AMD_MULTVAE_PHASES"] = "0"  # (read when a handle is made)
    plain = trainer_of(X, args)
    plain.run_epochs(1)  # (the first call of a process pays the code-object load)
    t0 = time.perf_counter()
    plain.run_epochs(args.epochs)
    wall = (time.perf_counter() - t0) / args.epochs
    epoch_ms = plain.stats()["epoch_ms"]
    plain.close()
    os.environ["IRSPACK_AMD_MULTVAE_PHASES"] = "1"
    timed = trainer_of(X, args)
    timed.run_epochs(2)
    st = timed.stats()
    timed.close()
    Hd, Hp = args.hidden, (args.hidden + 3) // 4 * 4
    big = 2.0 * U * I * (Hd + 1)  # flops of each of the three large products over an epoch
    atomics = (X.nnz * 0.5 + U) * Hp * 8.0  # kept entries (dropout 0.5) and the bias row, 8 bytes per element
    floor_ms = 3 * big / (ceiling * 1e9) + atomics / ATOMIC_GBS / 1e6
    out = dict(shape=args.shape, n_users=U, n_items=I, nnz=int(X.nnz), dim_z=args.dim_z, hidden=args.hidden,
               minibatch=args.minibatch, batches_per_epoch=st["batches_per_epoch"], dh2_slab=st["dh2_slab"],
               dw4_slab=st["dw4_slab"], scale_log2=st["scale_log2"], epoch_ms=round(epoch_ms, 2),
               wall_ms_per_epoch=round(wall * 1e3, 2), epoch_ms_with_phase_events=round(st["epoch_ms"], 2),
               **{k: round(st[k], 2) for k in ("encode_ms", "dense_ms", "logit_ms", "softmax_ms", "dw4_ms", "dh2_ms",
                                               "dw1_ms", "adam_ms")},
               logit_tflops=round(big / st["logit_ms"] / 1e9, 1), dw4_tflops=round(big / st["dw4_ms"] / 1e9, 1),
               dh2_tflops=round(big / st["dh2_ms"] / 1e9, 1), mfma_f32_ceiling_tflops=round(ceiling, 1),
               large_products_frac_of_ceiling=round(3 * big / ((st["logit_ms"] + st["dw4_ms"] + st["dh2_ms"]) * 1e9) / ceiling, 3),
               floor_ms=round(floor_ms, 2), launches_per_batch=19, nll_last=round(st["nll_last"], 4),
               kl_last=round(st["kl_last"], 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
