"""``MultVAERecommender`` (irspack/recommenders/multvae.py:293-380).  The reference trains with jax, haiku and optax
and draws its noise from jax's generator; here the trainer is the library's own statement of the same model
(``irs_multvae_*``): one tanh layer on each side, multinomial likelihood, annealed KL term,
Adam - with the order of an epoch, the dropout and the Gaussian noise drawn from a counter-based generator, so that
a fit is reproducible to the byte, also across ``save_state`` / ``load_state``."""
import ctypes as C
import pickle
from typing import IO, Any, Dict, Optional, Tuple

import numpy as np
import scipy.sparse as sps

from .. import _lib
from .._lib import check, lib, ptr, ptr_array
from ..optimization.parameter_range import CategoricalRange
from .base_earlystop import BaseRecommenderWithEarlyStopping, TrainerBase

TABLES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")
STATE_TABLES = TABLES + tuple("m" + n for n in TABLES) + tuple("v" + n for n in TABLES)


class MultVAETrainer(TrainerBase):
    """One ``irs_multvae`` handle: the eight float32 tables, their Adam moments and the update and epoch counters
    live on the device.  ``init`` (a dict of the eight tables) replaces the seeded initial values.  Nothing here
    needs a device until the first call that computes.

    ``l2_regularizer`` is accepted and stored and has no effect: the reference stores it (multvae.py:94, :103)
    and its loss never reads it (:189-200)."""

    def __init__(self, X: Any, dim_z: int, enc_hidden_dim: int, dec_hidden_dim: Optional[int], dropout_p: float,
                 l2_regularizer: float, kl_anneal_goal: float, anneal_end_epoch: int, minibatch_size: int,
                 learning_rate: float, random_seed: int = 42, device: Optional[int] = None,
                 init: Optional[Dict[str, np.ndarray]] = None) -> None:
        if dec_hidden_dim is None:
            dec_hidden_dim = enc_hidden_dim
        X = sps.csr_matrix(X)
        if not X.has_canonical_format:
            X = X.copy()
            X.sum_duplicates()
        self.X, indptr, indices, data = _lib.csr_arrays(X, np.float32)
        self.n_users, self.n_items = int(X.shape[0]), int(X.shape[1])
        self.hyper: Dict[str, Any] = dict(
            dim_z=int(dim_z), enc_hidden_dim=int(enc_hidden_dim), dec_hidden_dim=int(dec_hidden_dim),
            dropout_p=float(dropout_p), l2_regularizer=float(l2_regularizer), kl_anneal_goal=float(kl_anneal_goal),
            anneal_end_epoch=int(anneal_end_epoch), minibatch_size=int(minibatch_size),
            learning_rate=float(learning_rate), random_seed=int(random_seed))
        self.device = _lib.default_device() if device is None else int(device)
        self._h = C.c_void_p()
        self.version = 0  # counts the calls that changed the state (the recommender's host copies follow it)
        tables = None
        if init is not None:
            tables = [self._table(init, n) for n in TABLES]
        check(lib().irs_multvae_create(
            self.n_users, self.n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), ptr(data, C.c_float),
            int(dim_z), int(enc_hidden_dim), int(dec_hidden_dim), float(dropout_p), float(l2_regularizer),
            float(kl_anneal_goal), int(anneal_end_epoch), int(minibatch_size), float(learning_rate),
            C.c_uint64(int(random_seed) & (2 ** 64 - 1)), None if tables is None else ptr_array(tables, C.c_float),
            self.device, C.byref(self._h)))

    @property
    def shapes(self) -> Dict[str, Tuple[int, ...]]:
        I, H, Hd, L = self.n_items, self.hyper["enc_hidden_dim"], self.hyper["dec_hidden_dim"], self.hyper["dim_z"]
        return {"W1": (I, H), "b1": (H,), "W2": (H, 2 * L), "b2": (2 * L,), "W3": (L, Hd), "b3": (Hd,),
                "W4": (Hd, I), "b4": (I,)}

    def _table(self, source: Dict[str, Any], name: str) -> np.ndarray:
        a = np.ascontiguousarray(source[name], dtype=np.float32)
        want = self.shapes[name[-2:]]
        if a.shape != want:
            raise ValueError(f"table {name!r} has shape {a.shape}, expected {want}.")
        return a

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), C.c_void_p()
        if h is not None and h.value:
            lib().irs_multvae_destroy(h)

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
        check(lib().irs_multvae_run_epochs(self._h, int(n_epochs)))

    def order(self, epoch: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """the users that ``epoch`` takes at positions ``[first, first + count)``"""
        if count is None:
            count = self.n_users - int(first)
        users = np.zeros(max(int(count), 0), dtype=np.int32)
        check(lib().irs_multvae_order(self._h, int(epoch), int(first), int(count), ptr(users, C.c_int32)))
        return users

    def _users(self, users: Any) -> np.ndarray:
        return np.ascontiguousarray(users, dtype=np.int32).reshape(-1)

    def noise(self, update: int, users: Any) -> Tuple[np.ndarray, np.ndarray]:
        """``(keep, eps)`` of ``users`` at ``update``: one byte per stored entry, the rows in the order of ``users``,
        and ``(len(users), dim_z)`` Gaussians"""
        users = self._users(users)
        if users.size and (users.min() < 0 or users.max() >= self.n_users):
            raise ValueError("a batch row's user is out of range.")
        keep = np.zeros(int(np.diff(self.X.indptr)[users].sum()), dtype=np.uint8)
        eps = np.zeros((users.size, self.hyper["dim_z"]), dtype=np.float32)
        check(lib().irs_multvae_noise(self._h, int(update), users.size, ptr(users, C.c_int32), ptr(keep, C.c_uint8),
                                      ptr(eps, C.c_float)))
        return keep, eps

    def step_batch(self, users: Any, keep: Optional[Any] = None, eps: Optional[Any] = None,
                   klc: float = 0.0) -> Tuple[float, float]:
        """one update on the caller's rows with the caller's noise (``None``: drawn as ``run_epochs`` would at the
        current update count); returns the batch's mean NLL and mean KL"""
        users = self._users(users)
        if users.size and (users.min() < 0 or users.max() >= self.n_users):
            raise ValueError("a batch row's user is out of range.")
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)
            if keep.size != int(np.diff(self.X.indptr)[users].sum()):
                raise ValueError("keep must hold one value per stored entry of the batch's rows.")
        if eps is not None:
            eps = np.ascontiguousarray(eps, dtype=np.float32)
            if eps.shape != (users.size, self.hyper["dim_z"]):
                raise ValueError(f"eps has shape {eps.shape}, expected {(users.size, self.hyper['dim_z'])}.")
        nll, kl = C.c_double(0.0), C.c_double(0.0)
        self.version += 1
        check(lib().irs_multvae_step_batch(
            self._h, users.size, ptr(users, C.c_int32), None if keep is None else ptr(keep, C.c_uint8),
            None if eps is None else ptr(eps, C.c_float), float(klc), C.byref(nll), C.byref(kl)))
        return float(nll.value), float(kl.value)

    def gradients(self) -> Dict[str, np.ndarray]:
        """the eight gradient tables of the last update"""
        shapes = self.shapes
        grads = {n: np.zeros(shapes[n], dtype=np.float32) for n in TABLES}
        check(lib().irs_multvae_gradients(self._h, ptr_array([grads[n] for n in TABLES], C.c_float)))
        return grads

    def get_state(self) -> Dict[str, Any]:
        shapes = self.shapes
        state: Dict[str, Any] = {n: np.zeros(shapes[n[-2:]], dtype=np.float32) for n in STATE_TABLES}
        updates, epoch = C.c_int64(0), C.c_int64(0)
        check(lib().irs_multvae_get_state(self._h, ptr_array([state[n] for n in STATE_TABLES], C.c_float),
                                          C.byref(updates), C.byref(epoch)))
        state["n_updates"], state["epoch"] = int(updates.value), int(epoch.value)
        return state

    def set_state(self, state: Dict[str, Any]) -> None:
        tables = [self._table(state, n) for n in STATE_TABLES]
        self.version += 1
        check(lib().irs_multvae_set_state(self._h, ptr_array(tables, C.c_float), int(state["n_updates"]),
                                          int(state["epoch"])))

    def _rows(self, X: Any):
        X = sps.csr_matrix(X)
        if X.shape[1] != self.n_items:
            raise ValueError(f"the rows have {X.shape[1]} columns, the model has {self.n_items} items.")
        if not X.has_canonical_format:
            X = X.copy()
            X.sum_duplicates()
        return _lib.csr_arrays(X, np.float32)

    def encode(self, X: Any) -> Tuple[np.ndarray, np.ndarray]:
        """``(h2 (rows, Hd), lse (rows,))`` of the rows' evaluation forward pass: their log-softmax scores are
        ``[h2 | 1] @ [W4; b4] - lse``"""
        X, indptr, indices, data = self._rows(X)
        h2 = np.zeros((X.shape[0], self.hyper["dec_hidden_dim"]), dtype=np.float32)
        lse = np.zeros(X.shape[0], dtype=np.float32)
        check(lib().irs_multvae_encode(self._h, X.shape[0], ptr(indptr, C.c_int64), ptr(indices, C.c_int32),
                                       ptr(data, C.c_float), ptr(h2, C.c_float), ptr(lse, C.c_float)))
        return h2, lse

    def score(self, X: Any) -> np.ndarray:
        """float32 log-softmax scores of the rows (evaluation mode: no dropout, z = mu)"""
        X, indptr, indices, data = self._rows(X)
        out = np.zeros((X.shape[0], self.n_items), dtype=np.float32)
        check(lib().irs_multvae_score(self._h, X.shape[0], ptr(indptr, C.c_int64), ptr(indices, C.c_int32),
                                      ptr(data, C.c_float), ptr(out, C.c_float)))
        return out

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        return self.score(X).astype(np.float64)

    def stats(self) -> Dict[str, Any]:
        st = _lib.MultVaeStatsStruct()
        check(lib().irs_multvae_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in _lib.MultVaeStatsStruct._fields_ if name != "reserved"}

    # ---- base_earlystop.py's trainer contract --------------------------------------------------------------
    def save_state(self, ofs: IO) -> None:
        """the full state, the optimiser's included (the reference saves the parameters alone)"""
        pickle.dump(dict(self.get_state(), hyper=dict(self.hyper)), ofs, protocol=pickle.HIGHEST_PROTOCOL)

    def load_state(self, ifs: IO) -> None:
        state = pickle.load(ifs)
        if state.get("hyper", self.hyper) != self.hyper:
            raise ValueError(f"the saved state was trained with {state['hyper']}, this trainer has {self.hyper}.")
        self.set_state(state)


class MultVAERecommender(BaseRecommenderWithEarlyStopping):
    """multvae.py:329-380: the reference's arguments in the reference's order with the reference's defaults;
    ``random_seed`` and ``device`` are keyword extensions.  Scores are float64 log-softmax rows (:236).

    ``l2_regularizer`` is accepted and stored and has no effect, as in the reference (its loss never reads it).
    ``enc_hidden_dims`` and ``dec_hidden_dims`` are at most 574."""

    default_tune_range = [CategoricalRange("dim_z", [32, 64, 128, 256]),
                          CategoricalRange("enc_hidden_dims", [128, 256, 512]),
                          CategoricalRange("kl_anneal_goal", [0.1, 0.2, 0.4])]

    def __init__(self, X_train_all: Any, dim_z: int = 16, enc_hidden_dims: int = 256,
                 dec_hidden_dims: Optional[int] = None, dropout_p: float = 0.5, l2_regularizer: float = 0,
                 kl_anneal_goal: float = 0.2, anneal_end_epoch: int = 50, minibatch_size: int = 512,
                 train_epochs: int = 300, learning_rate: float = 1e-3, *, random_seed: int = 42,
                 device: Optional[int] = None) -> None:
        super().__init__(X_train_all, train_epochs=train_epochs)
        self.dim_z = dim_z
        self.enc_hidden_dims = enc_hidden_dims
        self.dec_hidden_dims = dec_hidden_dims
        self.kl_anneal_goal = kl_anneal_goal
        self.anneal_end_epoch = anneal_end_epoch
        self.minibatch_size = minibatch_size
        self.dropout_p = dropout_p
        self.l2_regularizer = l2_regularizer
        self.learning_rate = learning_rate
        self.random_seed = random_seed
        self.device = device
        self.trainer: Optional[MultVAETrainer] = None
        self._cached: Optional[Dict[str, Any]] = None

    def _create_trainer(self) -> MultVAETrainer:
        return MultVAETrainer(self.X_train_all, self.dim_z, self.enc_hidden_dims, self.dec_hidden_dims, self.dropout_p,
                              self.l2_regularizer, self.kl_anneal_goal, self.anneal_end_epoch, self.minibatch_size,
                              self.learning_rate, random_seed=self.random_seed, device=self.device)

    def _learn(self) -> None:
        # (no evaluator: the epochs go through one native call)
        self.start_learning()
        self.trainer.run_epochs(self.train_epochs)

    def _trained(self) -> MultVAETrainer:
        if self.trainer is None:
            raise RuntimeError("encoder called before training.")
        return self.trainer

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        return self.get_score_cold_user(self.X_train_all[user_indices])

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        return self.get_score_cold_user(self.X_train_all[begin:end])

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        return self._trained().get_score_cold_user(X)

    def factor_tables(self):
        """``([h2 | 1 | -lse], [W4; b4; 1])``: the model as a plain product of two float32 tables of ``Hd + 2``
        columns whose product is the log-softmax of every user's own row - the form the device evaluator and the
        serving layer take.  Held per state of the trainer."""
        trainer = self._trained()
        if self._cached is None or self._cached["_of"] != (id(trainer), trainer.version):
            version = trainer.version
            state = trainer.get_state()
            users = self.profile_factors(self.X_train_all)
            items = np.ascontiguousarray(np.concatenate(
                [state["W4"], state["b4"][None, :], np.ones((1, self.n_items), dtype=np.float32)], axis=0))
            self._cached = dict(_of=(id(trainer), version), tables=(users, items))
        return self._cached["tables"]

    def profile_factors(self, X: Any) -> np.ndarray:
        """``[h2 | 1 | -lse]`` of the rows of ``X``: the user side of ``factor_tables`` for new users"""
        h2, lse = self._trained().encode(X)
        return np.ascontiguousarray(np.concatenate(
            [h2, np.ones((h2.shape[0], 1), dtype=np.float32), -lse[:, None]], axis=1))
