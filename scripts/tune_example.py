"""The reference's example workflow (examples/movielens/movielens_1m.py:61-89) on a synthetic shape, ML-100K by
default: hold out half of every row, build an ``Evaluator`` on the validation half of the users' held-out entries and
one on the test half, ``tune`` every recommender class against the first, refit it with the best parameters and
score it against the second.

Where a trial's time goes is recorded on the way: per class and trial the wall time of the objective, split into
constructing and fitting the recommender (validations inside an early-stopping fit taken out), evaluating (those
validations and the final score), and the rest of ``tune`` (sampler, bookkeeping, the frame), which is charged to
the class as a whole.  One JSON line per trial, then one markdown table row per class.

    python scripts/tune_example.py [--shape ml100k] [--n-trials 8] [--classes IALSRecommender,...] [--seed 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import irspack_amd.recommenders as R  # noqa: E402
from irspack_amd.evaluation import Evaluator  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.utils import rowwise_train_test_split  # noqa: E402

DEFAULT_CLASSES = ["TopPopRecommender", "IALSRecommender", "DenseSLIMRecommender", "EDLAERecommender",
                   "SLIMRecommender", "CosineKNNRecommender", "AsymmetricCosineKNNRecommender",
                   "TverskyIndexKNNRecommender", "P3alphaRecommender", "RP3betaRecommender",
                   "CosineUserKNNRecommender", "TruncatedSVDRecommender", "NMFRecommender", "BPRFMRecommender",
                   "WARPFMRecommender", "MultVAERecommender"]


class TimedEvaluator:
    """an evaluator that adds up the time spent inside it"""

    def __init__(self, evaluator):
        self._evaluator = evaluator
        self.seconds = 0.0

    def __getattr__(self, name):
        return getattr(self._evaluator, name)

    def _timed(self, call, model):
        began = time.perf_counter()
        try:
            return call(model)
        finally:
            self.seconds += time.perf_counter() - began

    def get_score(self, model):
        return self._timed(self._evaluator.get_score, model)

    def get_target_score(self, model):
        return self._timed(self._evaluator.get_target_score, model)


def timed_class(cls, evaluator: TimedEvaluator, trials: list):
    """a subclass of ``cls`` that records, per instance that ``tune`` makes, the time to construct and fit it"""

    class Timed(cls):
        def __init__(self, *args, **kwargs):
            began = time.perf_counter()
            super().__init__(*args, **kwargs)
            # (what the evaluator has spent so far: a trial's evaluations lie between its mark and the next one's)
            self._record = dict(construct_fit_s=time.perf_counter() - began, evaluator_mark=evaluator.seconds)
            trials.append(self._record)

        def learn_with_optimizer(self, *args, **kwargs):
            began, inside = time.perf_counter(), evaluator.seconds
            try:
                return super().learn_with_optimizer(*args, **kwargs)
            finally:
                self._record["construct_fit_s"] += time.perf_counter() - began - (evaluator.seconds - inside)

    Timed.__name__ = cls.__name__
    return Timed


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml100k")
    ap.add_argument("--n-trials", type=int, default=8)
    ap.add_argument("--classes", default=",".join(DEFAULT_CLASSES))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    X = make_interactions(args.shape, dtype=np.float64)
    X_train, X_heldout = rowwise_train_test_split(X, test_ratio=0.5, random_state=args.seed)
    X_val, X_test = rowwise_train_test_split(X_heldout, test_ratio=0.5, random_state=args.seed + 1)
    validation, test = TimedEvaluator(Evaluator(X_val, cutoff=20)), Evaluator(X_test, cutoff=20)
    R.TopPopRecommender(X_train).learn()  # first use of the device
    test.get_score(R.TopPopRecommender(X_train).learn())

    rows = []
    for name in args.classes.split(","):
        cls, trials = getattr(R, name), []
        n_trials = args.n_trials if cls.default_tune_range else 1
        began = time.perf_counter()
        best, frame = timed_class(cls, validation, trials).tune(X_train, validation, n_trials=n_trials,
                                                                 tuning_random_seed=args.seed)
        wall = time.perf_counter() - began
        marks = [r["evaluator_mark"] for r in trials] + [validation.seconds]
        for number, record in enumerate(trials):
            objective = frame["duration"][number].total_seconds()
            record["evaluate_s"] = marks[number + 1] - marks[number]
            print(json.dumps(dict(recommender=name, trial=number, state=frame["state"][number],
                                  objective_s=round(objective, 6),
                                  construct_fit_s=round(record["construct_fit_s"], 6),
                                  evaluate_s=round(record["evaluate_s"], 6), value=frame["value"][number])))
        fit = sum(r["construct_fit_s"] for r in trials)
        evaluate = sum(r["evaluate_s"] for r in trials)
        refit = cls(X_train, **best).learn()
        scores = test.get_score(refit)
        rows.append(f"| {name} | {len(trials)} | {1e3 * wall / len(trials):.1f} | {1e3 * fit / len(trials):.1f} "
                    f"| {1e3 * evaluate / len(trials):.1f} | {1e3 * (wall - fit - evaluate) / len(trials):.1f} "
                    f"| {-frame['value'].min():.4f} | {scores['ndcg']:.4f} |")
    print(f"\nshape {args.shape}: {X.shape[0]} x {X.shape[1]}, {X.nnz} interactions; ms per trial, nDCG@20")
    print("| class | trials | wall | construct + fit | evaluate | rest | best validation nDCG | test nDCG |")
    print("|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main()
