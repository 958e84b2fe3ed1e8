"""``BPRFMRecommender`` (irspack/recommenders/bpr.py:23-184).  The reference wraps LightFM; here the trainer is the
library's own (``irs_bpr_*``): a synchronous mini-batch form of LightFM's per-sample step -
BPR loss, Adagrad, item biases - whose sampling, gradients and updates run on the device and are reproducible to
the byte.  The WARP loss (section 14, "WARP") is ``BPRFMTrainer(loss="warp")`` and ``WARPFMRecommender``;
``BPRFMRecommender(loss="warp")`` still refuses."""
import ctypes as C
import pickle
from typing import IO, Any, Dict, Optional

import numpy as np

from .. import _lib
from .._lib import check, lib, ptr
from .._threading import get_n_threads
from ..optimization.parameter_range import LogUniformFloatRange, UniformIntegerRange
from .base_earlystop import BaseRecommenderWithEarlyStopping, TrainerBase

_TABLES = ("U", "V", "b", "GU", "GV", "Gb")


class BPRFMTrainer(TrainerBase):
    """One ``irs_bpr`` handle: the six float32 tables and the epoch counter live on the device.  ``user_init`` /
    ``item_init`` replace the seeded initial embeddings.  Nothing here needs a device until the first call that
    computes or reads the state."""

    def __init__(self, X: Any, n_components: int, item_alpha: float, user_alpha: float, loss: str = "bpr",
                 n_threads: int = 1, learning_rate: float = 0.05, batch_size: int = 4096, random_seed: int = 42,
                 device: Optional[int] = None, user_init: Optional[np.ndarray] = None,
                 item_init: Optional[np.ndarray] = None, max_sampled: int = 10) -> None:
        if loss not in ("bpr", "warp"):
            raise ValueError('BPRFM loss must be either "bpr" or "warp".')
        self.loss = loss
        _, indptr, indices, data = _lib.csr_arrays(X, np.float32)
        self.n_users, self.n_items = int(X.shape[0]), int(X.shape[1])
        self.hyper: Dict[str, Any] = dict(
            n_components=int(n_components), item_alpha=float(item_alpha), user_alpha=float(user_alpha),
            learning_rate=float(learning_rate), batch_size=int(batch_size), random_seed=int(random_seed),
            loss=loss, max_sampled=int(max_sampled) if loss == "warp" else 0)
        self.n_threads = n_threads
        self.device = _lib.default_device() if device is None else int(device)
        self._h = C.c_void_p()
        self.version = 0  # counts the calls that changed the state (the recommender's host copies follow it)
        inits = []
        for table, rows in ((user_init, self.n_users), (item_init, self.n_items)):
            if table is not None:
                table = np.ascontiguousarray(table, dtype=np.float32)
                if table.shape != (rows, int(n_components)):
                    raise ValueError(f"an initial table has shape {table.shape}, expected {(rows, int(n_components))}.")
            inits.append(table)
        args = [self.n_users, self.n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), ptr(data, C.c_float),
                int(n_components), float(user_alpha), float(item_alpha), float(learning_rate), int(batch_size),
                C.c_uint64(int(random_seed) & (2 ** 64 - 1)), *(None if t is None else ptr(t, C.c_float) for t in inits),
                self.device]
        if loss == "warp":
            check(lib().irs_bpr_create_warp(*args, int(max_sampled), C.byref(self._h)))
        else:
            check(lib().irs_bpr_create(*args, C.byref(self._h)))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), C.c_void_p()
        if h is not None and h.value:
            lib().irs_bpr_destroy(h)

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    # ---- the native calls -------------------------------------------------------------------------------------
    def run_epoch(self) -> None:
        self.run_epochs(1)

    def run_epochs(self, n_epochs: int) -> None:
        self.version += 1
        check(lib().irs_bpr_run_epochs(self._h, int(n_epochs)))

    def sample(self, epoch: int, first: int = 0, count: Optional[int] = None):
        """the triples ``(users, positives, negatives)`` that ``epoch`` uses at positions ``[first, first + count)``"""
        if count is None:
            count = self.epoch_length - int(first)
        out = [np.zeros(max(int(count), 0), dtype=np.int32) for _ in range(3)]
        check(lib().irs_bpr_sample(self._h, int(epoch), int(first), int(count), *(ptr(a, C.c_int32) for a in out)))
        return tuple(out)

    def step_triples(self, users: Any, pos: Any, neg: Any) -> None:
        """one synchronous batch on the caller's triples"""
        arrays = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (users, pos, neg)]
        if not arrays[0].size == arrays[1].size == arrays[2].size:
            raise ValueError("users, pos and neg must have one length.")
        self.version += 1
        check(lib().irs_bpr_step_triples(self._h, arrays[0].size, *(ptr(a, C.c_int32) for a in arrays)))

    # ---- loss="warp" ----------------------------------------------------------------------------------------
    def candidates(self, epoch: int, first: int = 0, count: Optional[int] = None):
        """``(users, positives, cand)`` of ``epoch`` at positions ``[first, first + count)``; ``cand`` is
        ``count x max_sampled``, candidate ``t`` of a position in column ``t - 1``"""
        if count is None:
            count = self.epoch_length - int(first)
        n = max(int(count), 0)
        users, pos = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        cand = np.zeros((n, self.hyper["max_sampled"]), dtype=np.int32)
        check(lib().irs_bpr_warp_candidates(self._h, int(epoch), int(first), int(count),
                                            *(ptr(a, C.c_int32) for a in (users, pos, cand))))
        return users, pos, cand

    def _warp_batch(self, users: Any, pos: Any, cand: Any):
        users, pos = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (users, pos))
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        if users.size != pos.size or cand.shape != (users.size, self.hyper["max_sampled"]):
            raise ValueError("users and pos must have one length n, and cand the shape (n, max_sampled).")
        return users, pos, cand

    def search(self, users: Any, pos: Any, cand: Any):
        """the WARP search on the current state, nothing updated: ``(neg, tries)`` - per position the first
        candidate that violates the margin (-1: none) and the number of candidates examined"""
        users, pos, cand = self._warp_batch(users, pos, cand)
        neg, tries = np.zeros(users.size, dtype=np.int32), np.zeros(users.size, dtype=np.int32)
        check(lib().irs_bpr_warp_search(self._h, users.size, *(ptr(a, C.c_int32) for a in (users, pos, cand, neg, tries))))
        return neg, tries

    def step_candidates(self, users: Any, pos: Any, cand: Any) -> None:
        """one synchronous WARP batch on the caller's positions and candidates"""
        users, pos, cand = self._warp_batch(users, pos, cand)
        self.version += 1
        check(lib().irs_bpr_warp_step(self._h, users.size, *(ptr(a, C.c_int32) for a in (users, pos, cand))))

    def warp_stats(self) -> Dict[str, Any]:
        st = _lib.BprWarpStatsStruct()
        check(lib().irs_bpr_warp_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in _lib.BprWarpStatsStruct._fields_ if name != "reserved"}

    def get_state(self) -> Dict[str, Any]:
        k = self.hyper["n_components"]
        shapes = {"U": (self.n_users, k), "V": (self.n_items, k), "b": (self.n_items,)}
        state: Dict[str, Any] = {n: np.zeros(shapes[n.lstrip("G")], dtype=np.float32) for n in _TABLES}
        epoch = C.c_int64(0)
        check(lib().irs_bpr_get_state(self._h, *(ptr(state[n], C.c_float) for n in _TABLES), C.byref(epoch)))
        state["epoch"] = int(epoch.value)
        return state

    def set_state(self, state: Dict[str, Any]) -> None:
        k = self.hyper["n_components"]
        shapes = {"U": (self.n_users, k), "V": (self.n_items, k), "b": (self.n_items,)}
        tables = []
        for n in _TABLES:
            a = np.ascontiguousarray(state[n], dtype=np.float32)
            if a.shape != shapes[n.lstrip("G")]:
                raise ValueError(f"state[{n!r}] has shape {a.shape}, expected {shapes[n.lstrip('G')]}.")
            tables.append(a)
        self.version += 1
        check(lib().irs_bpr_set_state(self._h, *(ptr(a, C.c_float) for a in tables), int(state["epoch"])))

    def stats(self) -> Dict[str, Any]:
        st = _lib.BprStatsStruct()
        check(lib().irs_bpr_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in _lib.BprStatsStruct._fields_}

    @property
    def epoch_length(self) -> int:
        st = self.stats()
        return int(st["n_positives"] - st["n_skipped_positives"])

    # ---- base_earlystop.py's trainer contract --------------------------------------------------------------
    def save_state(self, ofs: IO) -> None:
        pickle.dump(dict(self.get_state(), hyper=dict(self.hyper)), ofs, protocol=pickle.HIGHEST_PROTOCOL)

    def load_state(self, ifs: IO) -> None:
        state = pickle.load(ifs)
        saved = state.get("hyper", self.hyper)
        # (a state saved before the trainer knew a loss is a BPR state)
        if dict(dict(loss="bpr", max_sampled=0), **saved) != self.hyper:
            raise ValueError(f"the saved state was trained with {saved}, this trainer has {self.hyper}.")
        self.set_state(state)


class BPRFMRecommender(BaseRecommenderWithEarlyStopping):
    """bpr.py:60-184: the reference's arguments in the reference's order; ``learning_rate``, ``batch_size``,
    ``random_seed`` and ``device`` are keyword extensions.  ``item_biases`` replaces ``fm.item_biases``."""

    # (bpr.py:100-105 without CategoricalRange("loss", ...): loss="warp" is WARPFMRecommender here, which inherits
    # the three ranges)
    default_tune_range = [UniformIntegerRange("n_components", 4, 256), LogUniformFloatRange("item_alpha", 1e-9, 1e-2),
                          LogUniformFloatRange("user_alpha", 1e-9, 1e-2)]

    def __init__(self, X_train_all: Any, n_components: int = 128, item_alpha: float = 1e-9, user_alpha: float = 1e-9,
                 loss: str = "bpr", n_threads: Optional[int] = None, train_epochs: int = 128, *,
                 learning_rate: float = 0.05, batch_size: int = 4096, random_seed: int = 42,
                 device: Optional[int] = None) -> None:
        super().__init__(X_train_all, train_epochs=train_epochs)
        self.n_components = n_components
        self.item_alpha = item_alpha
        self.user_alpha = user_alpha
        if loss not in {"bpr", "warp"}:
            raise ValueError('BPRFM loss must be either "bpr" or "warp".')
        if loss == "warp":
            raise NotImplementedError('BPRFM loss "warp" is not implemented on the device: use loss="bpr".')
        self.loss = loss
        self.trainer: Optional[BPRFMTrainer] = None
        self.n_threads = get_n_threads(n_threads)
        self.learning_rate = learning_rate
        self.batch_size = batch_size
        self.random_seed = random_seed
        self.device = device
        self._cached: Optional[Dict[str, Any]] = None

    def _create_trainer(self) -> BPRFMTrainer:
        return BPRFMTrainer(self.X_train_all, self.n_components, self.item_alpha, self.user_alpha, self.loss,
                            self.n_threads, learning_rate=self.learning_rate, batch_size=self.batch_size,
                            random_seed=self.random_seed, device=self.device)

    def _learn(self) -> None:
        # (no evaluator: the epochs go through one native call)
        self.start_learning()
        self.trainer.run_epochs(self.train_epochs)

    def _tables(self) -> Dict[str, Any]:
        """host copies of the trainer's tables, fetched once per state of the trainer"""
        trainer = self.trainer
        if trainer is None:
            raise RuntimeError("tried to fetch the embeddings before the fit.")
        if self._cached is None or self._cached["_of"] != (id(trainer), trainer.version):
            self._cached = dict(trainer.get_state(), _of=(id(trainer), trainer.version))
        return self._cached

    @property
    def item_biases(self) -> np.ndarray:
        return self._tables()["b"]

    def get_score(self, index: np.ndarray) -> np.ndarray:
        t = self._tables()
        return t["U"][index].dot(t["V"].T) + t["b"][np.newaxis, :]

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        t = self._tables()
        return t["U"][begin:end].dot(t["V"].T) + t["b"][np.newaxis, :]

    def get_user_embedding(self) -> np.ndarray:
        return self._tables()["U"]

    def get_score_from_user_embedding(self, user_embedding: np.ndarray) -> np.ndarray:
        t = self._tables()
        return user_embedding.dot(t["V"].T) + t["b"][np.newaxis, :]

    def get_item_embedding(self) -> np.ndarray:
        return self._tables()["V"]

    def get_score_from_item_embedding(self, user_indices: np.ndarray, item_embedding: np.ndarray) -> np.ndarray:
        # (without the bias, as in the reference)
        return self._tables()["U"][user_indices].dot(item_embedding.T)

    def factor_tables(self):
        """``([U | 1], [V | b]^T)``: the model as a plain product of two float32 tables of ``K + 1`` columns, the
        form the device evaluator and the serving layer take"""
        t = self._tables()
        held = t.get("_augmented")
        if held is None:
            users = np.concatenate([t["U"], np.ones((self.n_users, 1), dtype=np.float32)], axis=1)
            items = np.ascontiguousarray(np.concatenate([t["V"], t["b"][:, None]], axis=1).T)
            held = t["_augmented"] = (users, items)
        return held


class WARPFMRecommender(BPRFMRecommender):
    """The reference's ``BPRFMRecommender(loss="warp")`` (bpr.py:100-105) as a class of its own: the WARP ranking loss
    in the library's synchronous form ("WARP"), with ``max_sampled`` - for which the reference's
    constructor has no place - as a keyword.  Scoring, early stopping and the ``K + 1`` factor form are the parent's."""

    def __init__(self, X_train_all: Any, n_components: int = 128, item_alpha: float = 1e-9, user_alpha: float = 1e-9,
                 n_threads: Optional[int] = None, train_epochs: int = 128, *, max_sampled: int = 10,
                 learning_rate: float = 0.05, batch_size: int = 4096, random_seed: int = 42,
                 device: Optional[int] = None) -> None:
        super().__init__(X_train_all, n_components, item_alpha, user_alpha, "bpr", n_threads, train_epochs,
                         learning_rate=learning_rate, batch_size=batch_size, random_seed=random_seed, device=device)
        self.loss = "warp"
        self.max_sampled = max_sampled

    def _create_trainer(self) -> BPRFMTrainer:
        return BPRFMTrainer(self.X_train_all, self.n_components, self.item_alpha, self.user_alpha, "warp",
                            self.n_threads, learning_rate=self.learning_rate, batch_size=self.batch_size,
                            random_seed=self.random_seed, device=self.device, max_sampled=self.max_sampled)
