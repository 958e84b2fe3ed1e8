"""``BaseRecommenderWithEarlyStopping`` (irspack/recommenders/base_earlystop.py:52-149): recommenders that are
fitted epoch by epoch by a trainer object and can stop against a validation evaluator, reporting to a tuning
trial that may prune the fit.  The progress bar of the reference's loop is left out."""

from io import BytesIO
from typing import IO, Any, Optional

from .base import BaseRecommender


class TrainerBase:
    """base_earlystop.py:16-45: what the loop needs of a trainer."""

    def load_state(self, ifs: IO) -> None:
        raise NotImplementedError()

    def save_state(self, ofs: IO) -> None:
        raise NotImplementedError()

    def run_epoch(self) -> None:
        raise NotImplementedError()


class BaseRecommenderWithEarlyStopping(BaseRecommender):
    def __init__(self, X_train_all: Any, train_epochs: int = 128, **kwargs: Any) -> None:
        super().__init__(X_train_all, **kwargs)
        self.train_epochs = train_epochs
        self.trainer: Optional[Any] = None
        self.best_state: Optional[bytes] = None

    def _create_trainer(self) -> Any:
        raise NotImplementedError("_create_trainer must be implemented.")

    def _trainer_or_raise(self, caller: str) -> Any:
        trainer = getattr(self, "trainer", None)
        if trainer is None:  # base_earlystop.py:84-97
            raise RuntimeError(f"'{caller}' called before initializing the trainer.")
        return trainer

    # -- base_earlystop.py:80-149 ------------------------------------------
    def start_learning(self) -> None:
        self.trainer = self._create_trainer()

    def run_epoch(self) -> None:
        self._trainer_or_raise("run_epoch").run_epoch()

    def save_state(self) -> None:
        with BytesIO() as ofs:
            self._trainer_or_raise("save_state").save_state(ofs)
            self.best_state = ofs.getvalue()

    def load_state(self) -> None:
        if self.best_state is None:
            raise RuntimeError("'load_state' called before achieving any results.")
        with BytesIO(self.best_state) as ifs:
            self._trainer_or_raise("load_state").load_state(ifs)

    def _learn(self) -> None:
        self.learn_with_evaluator(None, max_epoch=self.train_epochs)

    def learn_with_evaluator(self, evaluator: Any, max_epoch: int = 128, validate_epoch: int = 5,
                             score_degradation_max: int = 5) -> None:
        """base_earlystop.py:106-149 without a trial: every ``validate_epoch`` epochs the evaluator
        scores the model; the best state is kept and restored at the end, and
        ``score_degradation_max`` validations in a row without a new best end the fit.
        ``evaluator=None``: exactly ``max_epoch`` epochs."""
        self.learn_with_optimizer(evaluator, None, max_epoch=max_epoch, validate_epoch=validate_epoch,
                                  score_degradation_max=score_degradation_max)

    def learn_with_optimizer(self, evaluator: Any, trial: Any, max_epoch: int = 128, validate_epoch: int = 5,
                             score_degradation_max: int = 5) -> None:
        """base_earlystop.py:106-149: the loop of ``learn_with_evaluator``; after every validation that did not
        end the fit, ``trial`` (if any) is told minus the score at the 0-based epoch and asked whether to go on:
        ``TrialPruned`` is raised if not."""
        self.start_learning()
        best, misses = -float("inf"), 0
        for done in range(1, max_epoch + 1):
            self.run_epoch()
            if evaluator is None or done % validate_epoch:
                continue
            score = evaluator.get_target_score(self)
            if score > best:
                best, misses = score, 0
                self.save_state()
                self.learnt_config["train_epochs"] = done
            else:
                misses += 1
                if misses >= score_degradation_max:
                    break
            if trial is not None:
                trial.report(-score, done - 1)
                if trial.should_prune():
                    from ..optimization.study import TrialPruned

                    raise TrialPruned()
        if evaluator is not None and self.best_state is not None:
            self.load_state()
