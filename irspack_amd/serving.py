"""Batch top-k recommendations from a trained model, on the device.

The reference serves through ``irspack.utils.IDMapper`` (utils/id_mapping.py:172-223, 399-453): a dense
``(n_users, n_items)`` score block on the host (``get_score_remove_seen``), then
``retrieve_recommend_from_score``.  ``DeviceRecommender`` keeps the model's item-side operand on the device
(``irs_serve_create_*``) and scores, excludes, ranks and emits ``(index, score)`` there (``irs_serve_recommend_*``):
the score block never leaves the device, three small arrays come home per call.

The model kinds are the ones the ``Evaluator`` scores on the device: sparse similarity weights (item-kNN, P3alpha,
RP3beta, SLIM: ``X_train[u] @ W``; user-kNN: ``U[u] @ X_train``) and dense ones (EASE, EDLAE) - the host product
bit for bit, float64 - and factor models (iALS, truncated SVD, NMF, BPR with its item bias as one more factor) -
float32 through the MFMA tiles.  A model whose
class overrides ``get_score_block`` scores some other way and is not recognised (``TypeError``).

``similar_items`` / ``similar_users`` rank the neighbours of items or users inside the resident operand
(``irs_serve_neighbors``): rows of ``W`` (or of the user-kNN ``U``) for similarity models, cosine or dot product of
the embedding tables for factor models.  Nothing in the reference corresponds to them.

The operands are copied when the ``DeviceRecommender`` is made: a model that is trained further needs a new one
(``irspack_amd.utils.IDMapper`` keeps one per model and notices).
"""

import ctypes as C
import weakref
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sps

from . import _lib
from ._lib import check, lib, ptr
from .recommenders.base import BaseRecommender

_SCORE_DTYPES = (np.float32, np.float64)
MAX_FACTORS = 576  # of irs_serve_create_factors

ArrayTriple = Tuple[np.ndarray, np.ndarray, np.ndarray]


def model_operands(model: Any) -> Optional[Tuple[str, Tuple[Any, ...]]]:
    """``(kind, operand objects)`` of a model the device can serve, ``None`` for any other.  Host only.

    kinds: ``"similarity"`` ``(X_train, W sparse)``, ``"user_similarity"`` ``(U, X_train)``, ``"dense_similarity"``
    ``(X_train, W ndarray)``, ``"factors"`` ``(user table (U, k), item table (k, I))`` and ``"ials"`` ``(trainer,)``.
    The rules are the Evaluator's (``_similarity_weights``, ``_dense_similarity_weights``, ``_factor_operands``, a
    trained iALS recommender): the class's own ``get_score_block`` must not be overridden."""
    from .recommenders.base import BaseSimilarityRecommender, BaseUserSimilarityRecommender
    from .recommenders.bpr import BPRFMRecommender
    from .recommenders.ials import IALSRecommender
    from .recommenders.multvae import MultVAERecommender
    from .recommenders.nmf import NMFRecommender
    from .recommenders.truncsvd import TruncatedSVDRecommender

    own = type(model).get_score_block if hasattr(type(model), "get_score_block") else None
    if isinstance(model, BaseSimilarityRecommender):
        if own is not BaseSimilarityRecommender.get_score_block:
            return None
        X, W = model.X_train_all, getattr(model, "_W", None)
        if not sps.issparse(X) or X.dtype != np.float64:
            return None
        if sps.issparse(W) and W.dtype in _SCORE_DTYPES and W.shape == (model.n_items, model.n_items):
            return "similarity", (X, W)
        if isinstance(W, np.ndarray) and W.dtype in _SCORE_DTYPES and W.flags.c_contiguous and \
                W.shape == (model.n_items, model.n_items):
            return "dense_similarity", (X, W)
        return None
    if isinstance(model, BaseUserSimilarityRecommender):
        if own is not BaseUserSimilarityRecommender.get_score_block:
            return None
        U, X = getattr(model, "U_", None), model.X_train_all
        if U is None or not sps.issparse(U) or U.dtype not in _SCORE_DTYPES or not sps.issparse(X) or \
                X.dtype != np.float64 or U.shape != (model.n_users, model.n_users):
            return None
        return "user_similarity", (U, X)
    if isinstance(model, (TruncatedSVDRecommender, NMFRecommender, BPRFMRecommender, MultVAERecommender)):
        if isinstance(model, MultVAERecommender):
            # [h2 | 1 | -lse] and [W4; b4; 1]: Hd + 2 columns, held by the model per trained state
            if own is not MultVAERecommender.get_score_block or model.trainer is None:
                return None
            users, items = model.factor_tables()
        elif isinstance(model, BPRFMRecommender):
            # [U | 1] and [V | b]^T: K + 1 columns, held by the model per trained state (a model that is trained
            # further hands out new tables, so both count as new operands)
            if own is not BPRFMRecommender.get_score_block or model.trainer is None:
                return None
            users, items = model.factor_tables()
        elif isinstance(model, TruncatedSVDRecommender):
            if own is not TruncatedSVDRecommender.get_score_block:
                return None
            users = getattr(model, "z_", None)
            items = getattr(getattr(model, "decomposer_", None), "components_", None)
        else:
            if own is not NMFRecommender.get_score_block:
                return None
            users, items = getattr(model, "W", None), getattr(model, "H", None)
        for F in (users, items):
            if not isinstance(F, np.ndarray) or F.ndim != 2 or F.dtype != np.float32:
                return None
        k = users.shape[1]
        if users.shape[0] != model.n_users or items.shape != (k, model.n_items) or not 1 <= k <= MAX_FACTORS:
            return None
        return "factors", (users, items)
    if isinstance(model, IALSRecommender):
        if own is not IALSRecommender.get_score_block:
            return None
        trainer = getattr(getattr(model, "trainer", None), "core_trainer", None)
        if trainer is None or not 1 <= int(model.n_components) <= MAX_FACTORS:
            return None
        return "ials", (trainer,)
    return None


def copied_operands(kind: str, operands: Tuple[Any, ...]) -> List[Any]:
    """the operands of ``model_operands`` whose CONTENT a ``DeviceRecommender`` copies when it is made - to the
    device, or into a converted host copy.  The others are read where they lie at every call (the training rows a
    call gathers, a user table that is already C-contiguous float32), so an edit of those in place needs no new
    device copy.  ``IDMapper`` fingerprints exactly the copied ones."""
    def read_in_place(M: Any) -> bool:  # (what _as_profile_rows returns unchanged)
        return sps.isspmatrix_csr(M) and M.dtype == np.float64

    if kind in ("similarity", "dense_similarity", "user_similarity"):
        rows, W = operands
        return [W] if read_in_place(rows) else [rows, W]
    if kind == "factors":
        users, items = operands
        return [items] if users.flags.c_contiguous else [users, items]
    return list(operands)  # iALS: both tables are downloaded from the trainer


def _canonical_rows(M: Any) -> sps.csr_matrix:
    """a float64 CSR COPY of sparse weights with sorted rows and no column stored twice (the model's matrix is
    never changed; float32 -> float64 is exact)"""
    out = sps.csr_matrix(M, dtype=np.float64, copy=True)
    out.sum_duplicates()
    out.sort_indices()
    return out


def _has_duplicate_columns(X: sps.csr_matrix) -> bool:
    """whether a row of the CSR matrix stores a column more than once"""
    if X.nnz < 2:
        return False
    if not X.has_sorted_indices:
        X = X.sorted_indices()
    same = X.indices[1:] == X.indices[:-1]
    if not same.any():
        return False
    row_start = np.zeros(X.nnz + 1, dtype=bool)
    row_start[X.indptr] = True  # (an equal pair across a row boundary is no duplicate)
    return bool((same & ~row_start[1:X.nnz]).any())


def _as_profile_rows(X: Any, n_cols: int) -> sps.csr_matrix:
    """the rows as CSR float64 in their STORAGE order (scipy's product adds a row's entries in that order)"""
    Xc = X if sps.isspmatrix_csr(X) else sps.csr_matrix(X)
    if Xc.dtype != np.float64:
        Xc = Xc.astype(np.float64)
    if Xc.shape[1] != n_cols:
        raise ValueError(f"profiles have {Xc.shape[1]} columns, the model expects {n_cols}.")
    return Xc


def _ragged(lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    lptr = np.zeros(len(lists) + 1, dtype=np.int64)
    for i, l in enumerate(lists):
        lptr[i + 1] = lptr[i] + len(l)
    items = np.zeros(max(int(lptr[-1]), 1), dtype=np.int64)
    for i, l in enumerate(lists):
        if len(l):
            items[lptr[i]:lptr[i + 1]] = np.asarray(l, dtype=np.int64)
    return lptr, items


def _exclusions(seen: sps.csr_matrix, forbidden: Optional[Sequence[Sequence[int]]],
                n_items: int) -> Tuple[np.ndarray, np.ndarray]:
    """CSR pattern of what a row must not be recommended: the NONZERO stored entries of ``seen`` (an explicit zero
    is not masked: ``scores[m.nonzero()] = -inf``, base.py:308-322) united with the row's forbidden indices"""
    rows = seen.shape[0]
    keep = seen.data != 0
    kept = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    indptr = kept[seen.indptr.astype(np.int64)]
    indices = seen.indices[keep].astype(np.int32)
    if forbidden is not None:
        if len(forbidden) != rows:
            raise ValueError("forbidden must hold one list per row.")
        parts, ptr_ = [], np.zeros(rows + 1, dtype=np.int64)
        for r in range(rows):
            f = np.asarray(forbidden[r], dtype=np.int64).reshape(-1)
            if f.size and (f.min() < 0 or f.max() >= n_items):
                raise ValueError("forbidden item index out of range.")
            parts.append(indices[indptr[r]:indptr[r + 1]])
            parts.append(f.astype(np.int32))
            ptr_[r + 1] = ptr_[r] + (indptr[r + 1] - indptr[r]) + f.size
        indptr = ptr_
        indices = np.concatenate(parts) if parts else indices[:0]
    return np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32)


def embedding_width(model: Any) -> int:
    """How many leading columns of a factor model's tables are the embedding (``k_used`` of
    ``irs_serve_neighbors``).  Host only; ``TypeError`` for a class without factor tables.

    BPR and WARP: ``n_components`` - the bias column of ``[V | b]`` and the 1 of ``[U | 1]`` do not count.
    Mult-VAE: the table width minus 2, the decoder's hidden width (``W4`` for items, ``h2`` for users; not ``b4``
    and 1, nor 1 and ``-lse``).  iALS, truncated SVD and NMF: the whole table, ``k``."""
    from .recommenders.bpr import BPRFMRecommender
    from .recommenders.ials import IALSRecommender
    from .recommenders.multvae import MultVAERecommender
    from .recommenders.nmf import NMFRecommender
    from .recommenders.truncsvd import TruncatedSVDRecommender

    if isinstance(model, MultVAERecommender):
        hidden = model.dec_hidden_dims if model.dec_hidden_dims is not None else model.enc_hidden_dims
        return int(hidden)
    if isinstance(model, (BPRFMRecommender, IALSRecommender)):
        return int(model.n_components)
    if isinstance(model, TruncatedSVDRecommender):
        components = getattr(getattr(model, "decomposer_", None), "components_", None)
        return int(components.shape[0] if components is not None else model.n_components)
    if isinstance(model, NMFRecommender):
        H = getattr(model, "H", None)
        return int(H.shape[0] if isinstance(H, np.ndarray) else model.n_components)
    raise TypeError(f"{type(model).__name__} has no embedding tables.")


_METRICS = {"weight": _lib.NEIGHBOR_WEIGHT, "cosine": _lib.NEIGHBOR_COSINE, "dot": _lib.NEIGHBOR_DOT}


class _Handle:
    """an ``irs_server`` that is destroyed with its last holder (a call keeps the one it runs on)"""

    def __init__(self) -> None:
        self.h = C.c_void_p()

    def close(self) -> None:
        h, self.h = self.h, C.c_void_p()
        if h.value:
            lib().irs_serve_destroy(h)

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


def arrays_to_lists(idx: np.ndarray, score: np.ndarray, length: np.ndarray) -> List[List[Tuple[int, float]]]:
    return [[(int(i), float(s)) for i, s in zip(idx[r, :length[r]], score[r, :length[r]])]
            for r in range(idx.shape[0])]


class DeviceRecommender:
    """Top-k lists for batches of users from a model whose item side stays on the device.

    ``recommend_known_arrays(user_indices, cutoff, ...)`` for users of the training matrix (seen items excluded),
    ``recommend_profiles_arrays(X, cutoff, ...)`` for new users given by their histories; both return
    ``(idx int32 (rows, width), score float32 (rows, width), length int32 (rows,))`` with
    ``width = min(cutoff, n_items)`` and ``-1`` / ``0`` in the padding; ``recommend_known`` / ``recommend_profiles``
    return lists of ``(index, score)``.  ``allowed`` is one list of candidate indices for every row,
    ``per_user_allowed`` one list per row (it takes precedence); order and duplicates are kept, indices outside
    ``[0, n_items)`` dropped.  ``forbidden`` is one list of indices per row.  Best first, no item whose score is
    ``-inf``, equal scores in candidate order (also on the host path that a profile row with a repeated column
    takes: a stable sort of the candidates).

    ``similar_items_arrays(item_indices, cutoff, ...)`` and ``similar_users_arrays(user_indices, cutoff, ...)``
    (``similar_items`` / ``similar_users`` for lists) rank the neighbours of each query entity among all items /
    users, the entity itself never among them; the lists are shaped like the recommend pair's, ``allowed`` /
    ``per_item_allowed`` / ``forbidden`` hold item indices on the item side and user indices on the user side.
    ``metric``: ``"weight"`` for similarity kinds (the stored weights of the row of ``W``, or of ``U`` for user-kNN;
    an entity without a stored weight in a sparse row is never listed), ``"cosine"`` (the default) or ``"dot"`` for
    factor kinds, over the embedding columns only (``embedding_width``).  The item side of a user-similarity model
    and the user side of an item-similarity model do not exist (``NotImplementedError``).  The user side has a
    device copy of its own (the user table, or ``U``), made at the first ``similar_users`` call: a snapshot like
    the item side's, dropped by ``drop_user_side()``.

    The model is needed at every call (its training rows, its new-user embedding).  ``weak_model=True`` keeps only
    a weak reference to it, for a holder whose entry must die with the model (``IDMapper``'s per-model cache): a
    call after the model is gone raises ``ReferenceError``.  The matrices and tables a call gathers rows from are
    kept by reference, not the model's operand tuple.

    One handle runs one device call at a time (the library serialises calls on it), so a ``DeviceRecommender``
    may be shared by threads; ``close()`` must not run beside a call."""

    def __init__(self, model: Any, device: Optional[int] = None, weak_model: bool = False) -> None:
        found = model_operands(model)
        if found is None:
            raise TypeError(f"{type(model).__name__} is not a model the device can serve: sparse or dense "
                            "similarity weights, truncated SVD, NMF or a trained iALS, BPR or Mult-VAE recommender, "
                            "scoring through its class's own get_score_block.")
        self.kind, operands = found
        self._model = weakref.ref(model) if weak_model else (lambda: model)
        self._model_name = type(model).__name__
        self.n_users, self.n_items = int(model.n_users), int(model.n_items)
        self.device = _lib.default_device() if device is None else int(device)
        self._h = C.c_void_p()
        self._users: Optional[np.ndarray] = None
        self._profiles: Optional[sps.csr_matrix] = None
        # (models without get_score_cold_user, as in the reference: user-kNN and BPR)
        self._cold_users = self.kind != "user_similarity" and \
            getattr(type(model), "get_score_cold_user", None) is not BaseRecommender.get_score_cold_user
        self._k_used = embedding_width(model) if self.kind in ("factors", "ials") else 0
        self._user_side: Optional[_Handle] = None
        self.user_side_key: Any = None  # (for a holder that watches the user-side operand: IDMapper)
        dev = C.c_int32(self.device)
        if self.kind in ("similarity", "user_similarity"):
            profiles, W = operands
            Wc = _canonical_rows(W)
            self._profiles = _as_profile_rows(profiles, Wc.shape[0])
            indptr = np.ascontiguousarray(Wc.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(Wc.indices, dtype=np.int32)
            data = np.ascontiguousarray(Wc.data, dtype=np.float64)
            check(lib().irs_serve_create_similarity(
                C.c_int64(Wc.shape[0]), C.c_int64(Wc.shape[1]), ptr(indptr, C.c_int64), ptr(indices, C.c_int32),
                ptr(data, C.c_double), dev, C.byref(self._h)))
        elif self.kind == "dense_similarity":
            profiles, W = operands
            self._profiles = _as_profile_rows(profiles, W.shape[0])
            check(lib().irs_serve_create_dense_similarity(
                C.c_int64(W.shape[0]), C.c_int64(W.shape[1]), C.c_int32(1 if W.dtype == np.float64 else 0),
                W.ctypes.data_as(C.c_void_p), dev, C.byref(self._h)))
        else:
            if self.kind == "ials":
                users, items = model.get_user_embedding(), model.get_item_embedding()
            else:
                users, items = operands[0], operands[1].T
            self._users = np.ascontiguousarray(users, dtype=np.float32)
            items = np.ascontiguousarray(items, dtype=np.float32)
            check(lib().irs_serve_create_factors(C.c_int64(items.shape[0]), C.c_int32(items.shape[1]),
                                                 ptr(items, C.c_float), dev, C.byref(self._h)))

    @property
    def model(self) -> Any:
        model = self._model()
        if model is None:
            raise ReferenceError(f"the {self._model_name} this DeviceRecommender served is gone.")
        return model

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), C.c_void_p()
        if h is not None and h.value:
            lib().irs_serve_destroy(h)
        self.drop_user_side()

    def drop_user_side(self) -> None:
        """lets go of the user-side device copy (the next ``similar_users`` call makes a new one); a call that
        still runs on it on another thread keeps it until it returns"""
        self._user_side = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    def last_phases(self) -> dict:
        """stream milliseconds of the last device call: upload, score, mask, rank (with the output stage)"""
        ms = (C.c_double * 4)()
        check(lib().irs_serve_last_phases(self._h, ms))
        return dict(zip(("upload", "score", "mask", "rank"), (float(v) for v in ms)))

    # ---- the two device calls -------------------------------------------------------------------------------
    def _lists(self, rows: int, allowed: Optional[Sequence[int]],
               per_user_allowed: Optional[Sequence[Sequence[int]]]) -> List[Sequence[int]]:
        if per_user_allowed is not None:
            if len(per_user_allowed) != rows:
                raise ValueError("per_user_allowed must hold one list per row.")
            return list(per_user_allowed)
        return [allowed] if allowed is not None else []

    def _outputs(self, rows: int, cutoff: int) -> ArrayTriple:
        width = max(min(int(cutoff), self.n_items), 0)
        return (np.full((rows, width), -1, dtype=np.int32), np.zeros((rows, width), dtype=np.float32),
                np.zeros(rows, dtype=np.int32))

    @staticmethod
    def _check_cutoff(cutoff: int) -> int:
        if int(cutoff) < 0:
            raise TypeError("cutoff must be non-negative (size_t).")
        return int(cutoff)

    def _call_profiles(self, P: sps.csr_matrix, excl: Tuple[np.ndarray, np.ndarray], lists: List[Sequence[int]],
                       cutoff: int) -> ArrayTriple:
        rows = P.shape[0]
        idx, score, length = self._outputs(rows, cutoff)
        if rows == 0:
            return idx, score, length
        lptr, litems = _ragged(lists)
        xp = np.ascontiguousarray(P.indptr, dtype=np.int64)
        xi = np.ascontiguousarray(P.indices, dtype=np.int32)
        xv = np.ascontiguousarray(P.data, dtype=np.float64)
        check(lib().irs_serve_recommend_profiles(
            self._h, C.c_int64(rows), ptr(xp, C.c_int64), ptr(xi, C.c_int32), ptr(xv, C.c_double),
            ptr(excl[0], C.c_int64), ptr(excl[1], C.c_int32), C.c_int64(len(lists)), ptr(lptr, C.c_int64),
            ptr(litems, C.c_int64), C.c_int64(cutoff), ptr(idx, C.c_int32), ptr(score, C.c_float),
            ptr(length, C.c_int32)))
        return idx, score, length

    def _call_factors(self, F: np.ndarray, excl: Tuple[np.ndarray, np.ndarray], lists: List[Sequence[int]],
                      cutoff: int) -> ArrayTriple:
        F = np.ascontiguousarray(F, dtype=np.float32)
        rows = F.shape[0]
        if F.ndim != 2 or F.shape[1] != self._users.shape[1]:
            raise ValueError("user factors have the wrong width.")
        idx, score, length = self._outputs(rows, cutoff)
        if rows == 0:
            return idx, score, length
        lptr, litems = _ragged(lists)
        check(lib().irs_serve_recommend_factors(
            self._h, C.c_int64(rows), ptr(F, C.c_float), ptr(excl[0], C.c_int64), ptr(excl[1], C.c_int32),
            C.c_int64(len(lists)), ptr(lptr, C.c_int64), ptr(litems, C.c_int64), C.c_int64(cutoff),
            ptr(idx, C.c_int32), ptr(score, C.c_float), ptr(length, C.c_int32)))
        return idx, score, length

    def _two_step(self, score: np.ndarray, lists: List[Sequence[int]], forbidden: Optional[Sequence[Sequence[int]]],
                  cutoff: int) -> ArrayTriple:
        """the host path: the model's own host scores (the reference's arithmetic kept exactly), ranked here by
        the rule of the device calls (util.hpp:426-504: candidates in list order, a STABLE sort by score so equal
        scores keep candidate order, the first ``cutoff`` of them up to the first -inf, float32 scores)"""
        score = np.asarray(score)
        if forbidden is not None:
            for r, f in enumerate(forbidden):
                score[r, np.asarray(f, dtype=np.int64).reshape(-1)] = -np.inf
        idx, sc, length = self._outputs(score.shape[0], cutoff)
        width = idx.shape[1]
        for r in range(score.shape[0]):
            if lists:
                cand = np.asarray(lists[0] if len(lists) == 1 else lists[r], dtype=np.int64).reshape(-1)
                cand = cand[(cand >= 0) & (cand < self.n_items)]
                row = score[r, cand]
            else:
                cand, row = None, score[r]
            best = np.argsort(-row, kind="stable")[:width]
            best = best[:int(np.argmax(np.append(row[best] == -np.inf, True)))]
            length[r] = best.size
            idx[r, :best.size] = best if cand is None else cand[best]
            sc[r, :best.size] = row[best]
        return idx, sc, length

    # ---- public ---------------------------------------------------------------------------------------------
    def recommend_known_arrays(self, user_indices: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                               per_user_allowed: Optional[Sequence[Sequence[int]]] = None,
                               forbidden: Optional[Sequence[Sequence[int]]] = None) -> ArrayTriple:
        cutoff = self._check_cutoff(cutoff)
        users = np.asarray(user_indices, dtype=np.int64).reshape(-1)
        if users.size and (users.min() < 0 or users.max() >= self.n_users):
            raise IndexError("user index out of range.")
        lists = self._lists(users.size, allowed, per_user_allowed)
        model = self.model
        seen = model.X_train_all[users].tocsr()
        if forbidden is not None and len(forbidden) != users.size:
            raise ValueError("forbidden must hold one list per row.")
        if self._users is not None:
            return self._call_factors(self._users[users], _exclusions(seen, forbidden, self.n_items), lists, cutoff)
        # (item-similarity models score from the rows they exclude: one gather)
        P = seen if self._profiles is model.X_train_all else self._profiles[users].tocsr()
        if _has_duplicate_columns(P):
            return self._two_step(model.get_score_remove_seen(users), lists, forbidden, cutoff)
        return self._call_profiles(P, _exclusions(seen, forbidden, self.n_items), lists, cutoff)

    def recommend_profiles_arrays(self, X: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                                  per_user_allowed: Optional[Sequence[Sequence[int]]] = None,
                                  forbidden: Optional[Sequence[Sequence[int]]] = None) -> ArrayTriple:
        cutoff = self._check_cutoff(cutoff)
        if not self._cold_users:
            raise NotImplementedError(f"get_score_cold_user is not implemented for {self._model_name}!")
        Xc = _as_profile_rows(X, self.n_items)
        lists = self._lists(Xc.shape[0], allowed, per_user_allowed)
        if forbidden is not None and len(forbidden) != Xc.shape[0]:
            raise ValueError("forbidden must hold one list per row.")
        if _has_duplicate_columns(Xc):
            return self._two_step(self.model.get_score_cold_user_remove_seen(Xc), lists, forbidden, cutoff)
        excl = _exclusions(Xc, forbidden, self.n_items)
        if self._users is None:
            return self._call_profiles(Xc, excl, lists, cutoff)
        if Xc.shape[0] == 0:
            return self._outputs(0, cutoff)
        if self.kind == "ials":
            F = self.model.compute_user_embedding(Xc)
        elif hasattr(self.model, "decomposer_"):
            F = self.model.decomposer.transform(Xc)  # X @ components_.T
        elif hasattr(self.model, "profile_factors"):
            F = self.model.profile_factors(Xc)  # Mult-VAE: [h2 | 1 | -lse] of the rows' own forward pass
        else:
            F = self.model.nmf_model.transform(Xc)  # nmf_transform
        return self._call_factors(F, excl, lists, cutoff)

    def recommend_known(self, user_indices: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                        per_user_allowed: Optional[Sequence[Sequence[int]]] = None,
                        forbidden: Optional[Sequence[Sequence[int]]] = None) -> List[List[Tuple[int, float]]]:
        return arrays_to_lists(*self.recommend_known_arrays(user_indices, cutoff, allowed, per_user_allowed, forbidden))

    def recommend_profiles(self, X: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                           per_user_allowed: Optional[Sequence[Sequence[int]]] = None,
                           forbidden: Optional[Sequence[Sequence[int]]] = None) -> List[List[Tuple[int, float]]]:
        return arrays_to_lists(*self.recommend_profiles_arrays(X, cutoff, allowed, per_user_allowed, forbidden))

    # ---- neighbours -----------------------------------------------------------------------------------------
    def user_side_arrays(self) -> List[np.ndarray]:
        """the host arrays the user-side device copy is a snapshot of (the user table; ``U`` of a user-kNN model)"""
        if self._users is not None:
            return [self._users]
        if self.kind == "user_similarity":
            return [self._profiles.indptr, self._profiles.indices, self._profiles.data]
        raise NotImplementedError(f"{self._model_name} has no user side to find neighbours in.")

    def _user_handle(self) -> _Handle:
        held = self._user_side
        if held is not None:
            return held
        held, dev = _Handle(), C.c_int32(self.device)
        if self._users is not None:
            users = self._users
            check(lib().irs_serve_create_factors(C.c_int64(users.shape[0]), C.c_int32(users.shape[1]),
                                                 ptr(users, C.c_float), dev, C.byref(held.h)))
        else:
            U = _canonical_rows(self._profiles)
            indptr = np.ascontiguousarray(U.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(U.indices, dtype=np.int32)
            data = np.ascontiguousarray(U.data, dtype=np.float64)
            check(lib().irs_serve_create_similarity(
                C.c_int64(U.shape[0]), C.c_int64(U.shape[1]), ptr(indptr, C.c_int64), ptr(indices, C.c_int32),
                ptr(data, C.c_double), dev, C.byref(held.h)))
        self._user_side = held
        return held

    def _metric_code(self, metric: Optional[str]) -> int:
        factor = self.kind in ("factors", "ials")
        if metric is None:
            metric = "cosine" if factor else "weight"
        if metric not in _METRICS:
            raise ValueError(f"metric must be one of {sorted(_METRICS)}, not {metric!r}.")
        if factor != (metric != "weight"):
            raise ValueError(f"metric {metric!r} does not fit a {self.kind} model: "
                             + ("'cosine' or 'dot'." if factor else "'weight'."))
        return _METRICS[metric]

    def _neighbors(self, h: C.c_void_p, n: int, what: str, indices: Any, cutoff: int,
                   allowed: Optional[Sequence[int]], per_row_allowed: Optional[Sequence[Sequence[int]]],
                   forbidden: Optional[Sequence[Sequence[int]]], metric: int) -> ArrayTriple:
        cutoff = self._check_cutoff(cutoff)
        ids = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise IndexError(f"{what} index out of range.")
        rows = int(ids.size)
        if per_row_allowed is not None:
            if len(per_row_allowed) != rows:
                raise ValueError(f"per_{what}_allowed must hold one list per row.")
            lists = list(per_row_allowed)
        else:
            lists = [allowed] if allowed is not None else []
        excl = _exclusions(sps.csr_matrix((rows, n), dtype=np.float64), forbidden, n)
        width = max(min(cutoff, n), 0)
        idx, score = np.full((rows, width), -1, dtype=np.int32), np.zeros((rows, width), dtype=np.float32)
        length = np.zeros(rows, dtype=np.int32)
        if rows == 0:
            return idx, score, length
        lptr, litems = _ragged(lists)
        check(lib().irs_serve_neighbors(
            h, C.c_int64(rows), ptr(ids, C.c_int64), C.c_int32(metric), C.c_int32(self._k_used),
            ptr(excl[0], C.c_int64), ptr(excl[1], C.c_int32), C.c_int64(len(lists)), ptr(lptr, C.c_int64),
            ptr(litems, C.c_int64), C.c_int64(cutoff), ptr(idx, C.c_int32), ptr(score, C.c_float),
            ptr(length, C.c_int32)))
        return idx, score, length

    def similar_items_arrays(self, item_indices: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                             per_item_allowed: Optional[Sequence[Sequence[int]]] = None,
                             forbidden: Optional[Sequence[Sequence[int]]] = None,
                             metric: Optional[str] = None) -> ArrayTriple:
        if self.kind == "user_similarity":
            raise NotImplementedError(f"{self._model_name} has no item side to find neighbours in.")
        return self._neighbors(self._h, self.n_items, "item", item_indices, cutoff, allowed, per_item_allowed,
                               forbidden, self._metric_code(metric))

    def similar_users_arrays(self, user_indices: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                             per_user_allowed: Optional[Sequence[Sequence[int]]] = None,
                             forbidden: Optional[Sequence[Sequence[int]]] = None,
                             metric: Optional[str] = None) -> ArrayTriple:
        if self.kind in ("similarity", "dense_similarity"):
            raise NotImplementedError(f"{self._model_name} has no user side to find neighbours in.")
        code = self._metric_code(metric)
        held = self._user_handle()  # (kept for the length of the call)
        return self._neighbors(held.h, self.n_users, "user", user_indices, cutoff, allowed, per_user_allowed,
                               forbidden, code)

    def similar_items(self, item_indices: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                      per_item_allowed: Optional[Sequence[Sequence[int]]] = None,
                      forbidden: Optional[Sequence[Sequence[int]]] = None,
                      metric: Optional[str] = None) -> List[List[Tuple[int, float]]]:
        return arrays_to_lists(*self.similar_items_arrays(item_indices, cutoff, allowed, per_item_allowed, forbidden,
                                                          metric))

    def similar_users(self, user_indices: Any, cutoff: int, allowed: Optional[Sequence[int]] = None,
                      per_user_allowed: Optional[Sequence[Sequence[int]]] = None,
                      forbidden: Optional[Sequence[Sequence[int]]] = None,
                      metric: Optional[str] = None) -> List[List[Tuple[int, float]]]:
        return arrays_to_lists(*self.similar_users_arrays(user_indices, cutoff, allowed, per_user_allowed, forbidden,
                                                          metric))
