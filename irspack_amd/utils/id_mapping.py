"""``ItemIDMapper`` / ``IDMapper`` (irspack/utils/id_mapping.py:51-453): recommendations by user and item ID.

Every public method, argument name, order and default is the reference's.  The single-user methods restate its
one-row host logic.  The two ``*_batch`` methods serve a model the device recognises through
``irspack_amd.serving.DeviceRecommender`` (kept per model, see ``_device_recommender``): scores, exclusions and
top-k stay on the device.  Any other model, and a batch below the model kind's ``DEVICE_MIN_BATCH``, takes the
reference's two steps - ``get_score_remove_seen`` / ``get_score_cold_user_remove_seen`` on the host, then
``retrieve_recommend_from_score`` (which orders equal scores inside an unsorted allowed list by item index; the
device path keeps them in the order of the list).

``ItemIDMapper.similar_items`` / ``similar_items_batch`` and ``IDMapper.similar_users`` / ``similar_users_batch``
have no counterpart in the reference: the neighbours of items or users by ID, ranked inside the model's resident
operand (``DeviceRecommender.similar_items`` / ``similar_users``), always on the device.
"""

import ctypes as C
import threading
import weakref
from typing import (TYPE_CHECKING, Any, Dict, Generic, Iterable, List, Optional, Sequence, Tuple, TypeVar, Union)

import numpy as np
import scipy.sparse as sps

from .._threading import get_n_threads
from . import retrieve_recommend_from_score

if TYPE_CHECKING:
    from ..recommenders.base import BaseRecommender

UserIdType = TypeVar("UserIdType")
ItemIdType = TypeVar("ItemIdType")
Profile = Union[List[ItemIdType], Dict[ItemIdType, float]]

# Per model kind (serving.model_operands): batches of fewer rows than this take the two-step path although the
# model is recognised.  A batch call through the mapper pays for the cache key (below) on top of the device call;
# the values are the crossovers scripts/serve_bench.py measured for the mapper's own call, DESIGN.md section 13.
# Similarity models win at one user already.  iALS pays ~6 ms per call to bring both tables home for the key: its
# mapper call loses at 64 users (6.2 ms against 5.6 ms) and wins at 1,024 (11.7 against 30.2 ms); straight lines
# through those points meet near 95 users.
DEVICE_MIN_BATCH: Dict[str, int] = {"similarity": 0, "user_similarity": 0, "dense_similarity": 0, "factors": 0,
                                    "ials": 128}


class _Held:
    """what the cache keeps for one model: the key its device copy was made from, the copy, and the finalizer that
    closes the copy when the model is collected"""
    __slots__ = ("key", "served", "closer")

    def __init__(self, key: Tuple[Any, ...], served: Any, closer: Any) -> None:
        self.key, self.served, self.closer = key, served, closer


# model -> _Held.  The entry must die with its model, so nothing in it may reference the model strongly: the
# DeviceRecommender is made with weak_model=True.  `_cache_lock` guards lookups and replacements (two threads
# serving one model share one entry; the device calls themselves are serialised inside the handle).
_recommenders: "weakref.WeakKeyDictionary[Any, _Held]" = weakref.WeakKeyDictionary()
_cache_lock = threading.Lock()


def _fingerprint(a: np.ndarray) -> int:
    from .._lib import check, lib

    a = np.ascontiguousarray(a)
    out = C.c_uint64(0)
    check(lib().irs_fingerprint(a.ctypes.data_as(C.c_void_p) if a.size else None, C.c_int64(a.nbytes),
                                C.c_uint64(0), C.byref(out)))
    return int(out.value)


def _operand_key(kind: str, operands: Tuple[Any, ...]) -> Tuple[Any, ...]:
    """Identity and shape of every operand object, plus the content fingerprint of the buffers the device copy was
    made FROM (``serving.copied_operands``: the item-side weights or tables, and whatever had to be converted):
    a model that was trained further, or whose weights were edited in place, gets a new device copy.  Operands
    that every call reads where they lie (CSR float64 training rows) need no fingerprint.  The cost is per batch
    call: one pass over the copied buffers on the host's threads (the 2.9 GB of an ML-20M EASE ``W``), for iALS
    also the download of both factor tables from the trainer."""
    from ..serving import copied_operands

    key: List[Any] = [kind]
    for op in operands:
        key += [id(op), getattr(op, "shape", None)]
    for op in copied_operands(kind, operands):
        if sps.issparse(op):
            key += [_fingerprint(op.indptr), _fingerprint(op.indices), _fingerprint(op.data)]
        elif isinstance(op, np.ndarray):
            key.append(_fingerprint(op))
        else:  # an iALS trainer: both factor tables
            key += [_fingerprint(op.user), _fingerprint(op.item)]
    return tuple(key)


def _device_recommender(recommender: Any, n_rows: int, new_users: bool = False) -> Optional[Any]:
    """The model's ``DeviceRecommender`` (made once, remade when the operands changed); ``None`` for a model the
    device does not recognise, for a batch below the kind's ``DEVICE_MIN_BATCH`` and for new users of a
    user-similarity model (which has no such path).  A copy that is replaced is
    only let go of here: it closes itself when its last user (a call still running on another thread) drops it."""
    from .. import serving

    found = serving.model_operands(recommender)
    if found is None or n_rows < max(DEVICE_MIN_BATCH.get(found[0], 0), 1):
        return None
    if new_users and found[0] == "user_similarity":
        return None
    key = _operand_key(*found)
    with _cache_lock:
        try:
            held = _recommenders.get(recommender)
        except TypeError:  # (no weak references to this object: nothing is kept)
            return serving.DeviceRecommender(recommender)
        if held is not None and held.key == key:
            return held.served
        if held is not None:
            held.closer.detach()
        served = serving.DeviceRecommender(recommender, weak_model=True)
        closer = weakref.finalize(recommender, served.close)
        closer.atexit = False  # (at interpreter exit the handle goes with the process)
        _recommenders[recommender] = _Held(key, served, closer)
        return served


def _neighbour_recommender(recommender: Any, n_rows: int, user_side: bool = False) -> Any:
    """The model's cached ``DeviceRecommender`` for a neighbour call, whatever the batch size: these calls have no
    host path, so a model the device does not recognise raises ``DeviceRecommender``'s ``TypeError``.  The user
    side has a device copy of its own, made at its first use; the operand it was made from (the user table, or the
    ``U`` of a user-kNN model) is read in place by every other call and so is no part of the per-call key:
    its fingerprint is taken here, and the copy is let go of when it differs from the one taken when the copy was
    made."""
    from .. import serving

    found = serving.model_operands(recommender)
    if found is None:
        return serving.DeviceRecommender(recommender)  # (raises)
    dev = _device_recommender(recommender, max(n_rows, DEVICE_MIN_BATCH.get(found[0], 0), 1))
    if user_side and found[0] not in ("similarity", "dense_similarity"):
        key = tuple(_fingerprint(a) for a in dev.user_side_arrays())
        with _cache_lock:
            if dev.user_side_key != key:
                dev.drop_user_side()
                dev.user_side_key = key
    return dev


class ItemIDMapper(Generic[ItemIdType]):
    """Translates between item IDs and the item indices of a recommender or a score array
    (irspack/utils/id_mapping.py:51-325).

    ``item_ids[i]`` is the ID of item index ``i``: the list must be in the order of the columns of the training
    matrix.  IDs are dictionary keys, so they must be hashable; a repeated ID raises ``ValueError``.
    """

    def __init__(self, item_ids: List[ItemIdType]):  # id_mapping.py:64-71
        self.item_ids = item_ids
        self.item_id_to_index = {iid: index for index, iid in enumerate(item_ids)}
        if len(self.item_id_to_index) != len(item_ids):
            raise ValueError("Duplicates in item_ids.")

    def _require_n_items(self, recommender: "BaseRecommender") -> None:  # id_mapping.py:73-75
        if recommender.n_items != len(self.item_ids):
            raise ValueError("`n_items` of the recommender is inconsistent.")

    def _require_score_width(self, score: np.ndarray) -> None:  # id_mapping.py:77-79
        if score.shape[1] != len(self.item_ids):
            raise ValueError("`score.shape[1]` inconsistent with `len(self.item_ids)`")

    def _known_indices(self, ids: Iterable[ItemIdType]) -> List[int]:
        """indices of the IDs this mapper knows, in the order given; unknown IDs are dropped (id_mapping.py:81-82)"""
        lookup = self.item_id_to_index
        return [lookup[iid] for iid in ids if iid in lookup]

    def _profile_entries(self, profile: Profile) -> Tuple[List[int], List[float]]:
        """``(columns, values)`` of one profile in its own order: a list of IDs counts 1.0 each, a dict gives the
        ratings (a rating of 0.0 stays an entry); unknown IDs are dropped (id_mapping.py:84-100)"""
        if isinstance(profile, list):
            columns = self._known_indices(profile)
            return columns, [1.0] * len(columns)
        known = [(self.item_id_to_index[iid], rating) for iid, rating in profile.items()
                 if iid in self.item_id_to_index]
        return [c for c, _ in known], [r for _, r in known]

    def list_of_user_profile_to_matrix(self, users_info: Sequence[Profile]) -> sps.csr_matrix:
        """One CSR float64 row per profile (a list of item IDs, or an item ID -> rating dict), the columns those of
        ``self.item_ids`` (id_mapping.py:102-129).  Unknown IDs are dropped, entries keep the order of the
        profile, a rating of 0.0 stays a stored zero."""
        columns: List[int] = []
        values: List[float] = []
        row_ends = [0]
        for profile in users_info:
            c, v = self._profile_entries(profile)
            columns += c
            values += v
            row_ends.append(len(columns))
        return sps.csr_matrix((np.asarray(values, dtype=np.float64), np.asarray(columns, dtype=np.int32),
                               np.asarray(row_ends, dtype=np.int32)), shape=(len(users_info), len(self.item_ids)))

    def recommend_for_new_user(
        self,
        recommender: "BaseRecommender",
        user_profile: Union[List[ItemIdType], Dict[ItemIdType, float]],
        cutoff: int = 20,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        forbidden_item_ids: Optional[List[ItemIdType]] = None,
    ) -> List[Tuple[ItemIdType, float]]:
        """``(item_id, score)`` pairs, best first, for a user the model has not seen, from the user's history
        (id_mapping.py:131-170).  One row on the host: ``get_score_cold_user_remove_seen``, then
        ``score_to_recommended_items``."""
        self._require_n_items(recommender)
        row = self.list_of_user_profile_to_matrix([user_profile])
        score = recommender.get_score_cold_user_remove_seen(row)[0]
        return self.score_to_recommended_items(score, cutoff, allowed_item_ids=allowed_item_ids,
                                               forbidden_item_ids=forbidden_item_ids)

    def _batch_lists_as_indices(
        self, n_rows: int,
        allowed_item_ids: Optional[List[ItemIdType]],
        per_user_allowed_item_ids: Optional[List[List[ItemIdType]]],
        forbidden_item_ids: Optional[List[List[ItemIdType]]],
    ) -> Tuple[Optional[List[int]], Optional[List[List[int]]], Optional[List[List[int]]]]:
        """``(allowed, per-row allowed, per-row forbidden)`` as index lists; the per-row allowed lists take
        precedence over the common one (id_mapping.py:292-311)"""
        if forbidden_item_ids is not None:
            assert len(forbidden_item_ids) == n_rows
        if per_user_allowed_item_ids is not None:
            assert len(per_user_allowed_item_ids) == n_rows
        allowed = per_user = forbidden = None
        if per_user_allowed_item_ids is not None:
            per_user = [self._known_indices(ids) for ids in per_user_allowed_item_ids]
        elif allowed_item_ids is not None:
            allowed = self._known_indices(allowed_item_ids)
        if forbidden_item_ids is not None:
            forbidden = [self._known_indices(ids) for ids in forbidden_item_ids]
        return allowed, per_user, forbidden

    def _arrays_to_id_lists(self, idx: np.ndarray, score: np.ndarray,
                            length: np.ndarray) -> List[List[Tuple[ItemIdType, float]]]:
        return [[(self.item_ids[int(i)], float(s)) for i, s in zip(idx[r, :length[r]], score[r, :length[r]])]
                for r in range(idx.shape[0])]

    def recommend_for_new_user_batch(
        self,
        recommender: "BaseRecommender",
        user_profiles: Sequence[Union[List[ItemIdType], Dict[ItemIdType, float]]],
        cutoff: int = 20,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        per_user_allowed_item_ids: Optional[List[List[ItemIdType]]] = None,
        forbidden_item_ids: Optional[List[List[ItemIdType]]] = None,
        n_threads: Optional[int] = None,
    ) -> List[List[Tuple[ItemIdType, float]]]:
        """One best-first list of ``(item_id, score)`` per profile, for users the model has not seen
        (id_mapping.py:172-223).  ``per_user_allowed_item_ids`` wins over ``allowed_item_ids``.  A recognised
        model is served on the device; ``n_threads`` matters to the two-step path only."""
        self._require_n_items(recommender)
        X_input = self.list_of_user_profile_to_matrix(user_profiles)
        dev = _device_recommender(recommender, X_input.shape[0], new_users=True)
        if dev is not None:
            allowed, per_user, forbidden = self._batch_lists_as_indices(
                X_input.shape[0], allowed_item_ids, per_user_allowed_item_ids, forbidden_item_ids)
            return self._arrays_to_id_lists(
                *dev.recommend_profiles_arrays(X_input, cutoff, allowed, per_user, forbidden))
        score = recommender.get_score_cold_user_remove_seen(X_input)
        return self.score_to_recommended_items_batch(
            score, cutoff, allowed_item_ids=allowed_item_ids, per_user_allowed_item_ids=per_user_allowed_item_ids,
            forbidden_item_ids=forbidden_item_ids, n_threads=get_n_threads(n_threads=n_threads))

    def similar_items(
        self,
        recommender: "BaseRecommender",
        item_id: ItemIdType,
        cutoff: int = 20,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        forbidden_item_ids: Optional[List[ItemIdType]] = None,
        metric: Optional[str] = None,
    ) -> List[Tuple[ItemIdType, float]]:
        """``(item_id, score)`` pairs, best first, of the items most like ``item_id`` in the model - never the item
        itself (no counterpart in the reference; ``DeviceRecommender.similar_items``).  Always on the device.  An
        ID that is not in ``self.item_ids`` raises ``RuntimeError``; unknown IDs inside the lists are dropped."""
        return self.similar_items_batch(
            recommender, [item_id], cutoff=cutoff, allowed_item_ids=allowed_item_ids,
            forbidden_item_ids=None if forbidden_item_ids is None else [forbidden_item_ids], metric=metric)[0]

    def similar_items_batch(
        self,
        recommender: "BaseRecommender",
        item_ids: List[ItemIdType],
        cutoff: int = 20,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        per_item_allowed_item_ids: Optional[List[List[ItemIdType]]] = None,
        forbidden_item_ids: Optional[List[List[ItemIdType]]] = None,
        metric: Optional[str] = None,
    ) -> List[List[Tuple[ItemIdType, float]]]:
        """One best-first list of ``(item_id, score)`` per query item ID.  ``per_item_allowed_item_ids`` wins over
        ``allowed_item_ids``; ``metric`` as in ``DeviceRecommender.similar_items``."""
        self._require_n_items(recommender)
        for iid in item_ids:
            if iid not in self.item_id_to_index:
                raise RuntimeError(f"Item with item_id {iid} not found.")
        rows = np.asarray([self.item_id_to_index[iid] for iid in item_ids], dtype=np.int64)
        dev = _neighbour_recommender(recommender, rows.size)
        allowed, per_item, forbidden = self._batch_lists_as_indices(
            rows.size, allowed_item_ids, per_item_allowed_item_ids, forbidden_item_ids)
        return self._arrays_to_id_lists(
            *dev.similar_items_arrays(rows, cutoff, allowed, per_item, forbidden, metric))

    def score_to_recommended_items(
        self,
        score: np.ndarray,
        cutoff: int,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        forbidden_item_ids: Optional[List[ItemIdType]] = None,
    ) -> List[Tuple[ItemIdType, float]]:
        """``(item_id, score)`` pairs from ONE row of scores, on the host (id_mapping.py:225-256): the candidates
        (all items, or the known allowed ones) by ``argsort()[::-1]``, skipping infinite scores of either sign and
        IDs in ``forbidden_item_ids``, until ``cutoff`` pairs are collected."""
        self._require_score_width(score[None, :])
        if allowed_item_ids is None:
            ranked = score.argsort()[::-1]
        else:
            candidates = np.asarray(self._known_indices(allowed_item_ids), dtype=np.int64)
            ranked = candidates[score[candidates].argsort()[::-1]]
        picked: List[Tuple[ItemIdType, float]] = []
        for index in map(int, ranked):
            value = score[index]
            if np.isinf(value):
                continue
            iid = self.item_ids[index]
            if forbidden_item_ids is not None and iid in forbidden_item_ids:
                continue
            picked.append((iid, float(value)))
            if len(picked) >= cutoff:  # (checked after the append, as the reference does)
                break
        return picked

    def score_to_recommended_items_batch(
        self,
        score: np.ndarray,
        cutoff: int,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        per_user_allowed_item_ids: Optional[List[List[ItemIdType]]] = None,
        forbidden_item_ids: Optional[List[List[ItemIdType]]] = None,
        n_threads: Optional[int] = None,
    ) -> List[List[Tuple[ItemIdType, float]]]:
        """Lists from a host score array, float32 or float64, ``(rows, len(item_ids))`` (id_mapping.py:258-325).
        An item whose score is ``-inf`` is not recommended.  The forbidden items of a row are set to ``-inf`` IN
        the caller's array, as the reference does."""
        self._require_score_width(score)
        allowed, per_user, forbidden = self._batch_lists_as_indices(
            score.shape[0], allowed_item_ids, per_user_allowed_item_ids, forbidden_item_ids)
        lists: List[List[int]] = per_user if per_user is not None else ([allowed] if allowed is not None else [])
        if forbidden is not None:
            for row, indices in enumerate(forbidden):
                score[row, indices] = -np.inf
        ranked = retrieve_recommend_from_score(score, lists, cutoff, n_threads=get_n_threads(n_threads))
        return [[(self.item_ids[index], value) for index, value in row] for row in ranked]


class IDMapper(Generic[UserIdType, ItemIdType], ItemIDMapper[ItemIdType]):
    """``ItemIDMapper`` plus the user side (irspack/utils/id_mapping.py:327-453): ``user_ids[u]`` is the ID of
    user index ``u``, in the order of the rows of the training matrix.  A repeated user or item ID raises
    ``ValueError``.
    """

    def __init__(self, user_ids: List[UserIdType], item_ids: List[ItemIdType]):  # id_mapping.py:343-348
        super().__init__(item_ids)
        self.user_ids = user_ids
        self.user_id_to_index = {uid: index for index, uid in enumerate(user_ids)}
        if len(self.user_id_to_index) != len(user_ids):
            raise ValueError("Duplicates in user_ids.")

    def _require_n_users(self, recommender: "BaseRecommender") -> None:  # id_mapping.py:350-352
        if recommender.n_users != len(self.user_ids):
            raise ValueError("`n_users` of the recommender is inconsistent.")

    def recommend_for_known_user_id(
        self,
        recommender: "BaseRecommender",
        user_id: UserIdType,
        cutoff: int = 20,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        forbidden_item_ids: Optional[List[ItemIdType]] = None,
    ) -> List[Tuple[ItemIdType, float]]:
        """``(item_id, score)`` pairs, best first, for one user of the training matrix, seen items left out
        (id_mapping.py:354-397).  One row on the host.  An ID that is not in ``self.user_ids`` raises
        ``RuntimeError``."""
        self._require_n_users(recommender)
        if user_id not in self.user_id_to_index:
            raise RuntimeError(f"User with user_id {user_id} not found.")
        row = np.asarray([self.user_id_to_index[user_id]], dtype=np.int64)
        score = recommender.get_score_remove_seen(row)[0, :]
        return self.score_to_recommended_items(score, cutoff=cutoff, allowed_item_ids=allowed_item_ids,
                                               forbidden_item_ids=forbidden_item_ids)

    def recommend_for_known_user_batch(
        self,
        recommender: "BaseRecommender",
        user_ids: List[UserIdType],
        cutoff: int = 20,
        allowed_item_ids: Optional[List[ItemIdType]] = None,
        per_user_allowed_item_ids: Optional[List[List[ItemIdType]]] = None,
        forbidden_item_ids: Optional[List[List[ItemIdType]]] = None,
        n_threads: Optional[int] = None,
    ) -> List[List[Tuple[ItemIdType, float]]]:
        """One best-first list of ``(item_id, score)`` per user ID, seen items left out (id_mapping.py:399-453).
        ``per_user_allowed_item_ids`` wins over ``allowed_item_ids``.  A recognised model is served on the device;
        ``n_threads`` matters to the two-step path only."""
        self._require_n_users(recommender)
        rows = np.asarray([self.user_id_to_index[uid] for uid in user_ids], dtype=np.int64)
        dev = _device_recommender(recommender, rows.size)
        if dev is not None:
            allowed, per_user, forbidden = self._batch_lists_as_indices(
                rows.size, allowed_item_ids, per_user_allowed_item_ids, forbidden_item_ids)
            return self._arrays_to_id_lists(*dev.recommend_known_arrays(rows, cutoff, allowed, per_user, forbidden))
        score = recommender.get_score_remove_seen(rows)
        return self.score_to_recommended_items_batch(
            score, cutoff=cutoff, allowed_item_ids=allowed_item_ids,
            per_user_allowed_item_ids=per_user_allowed_item_ids, forbidden_item_ids=forbidden_item_ids,
            n_threads=get_n_threads(n_threads=n_threads))

    def _known_user_indices(self, ids: Iterable[UserIdType]) -> List[int]:
        """indices of the user IDs this mapper knows, in the order given; unknown IDs are dropped"""
        lookup = self.user_id_to_index
        return [lookup[uid] for uid in ids if uid in lookup]

    def similar_users(
        self,
        recommender: "BaseRecommender",
        user_id: UserIdType,
        cutoff: int = 20,
        allowed_user_ids: Optional[List[UserIdType]] = None,
        forbidden_user_ids: Optional[List[UserIdType]] = None,
        metric: Optional[str] = None,
    ) -> List[Tuple[UserIdType, float]]:
        """``(user_id, score)`` pairs, best first, of the users most like ``user_id`` in the model - never the user
        itself (no counterpart in the reference; ``DeviceRecommender.similar_users``).  Always on the device.  An
        ID that is not in ``self.user_ids`` raises ``RuntimeError``; unknown IDs inside the lists are dropped."""
        return self.similar_users_batch(
            recommender, [user_id], cutoff=cutoff, allowed_user_ids=allowed_user_ids,
            forbidden_user_ids=None if forbidden_user_ids is None else [forbidden_user_ids], metric=metric)[0]

    def similar_users_batch(
        self,
        recommender: "BaseRecommender",
        user_ids: List[UserIdType],
        cutoff: int = 20,
        allowed_user_ids: Optional[List[UserIdType]] = None,
        per_user_allowed_user_ids: Optional[List[List[UserIdType]]] = None,
        forbidden_user_ids: Optional[List[List[UserIdType]]] = None,
        metric: Optional[str] = None,
    ) -> List[List[Tuple[UserIdType, float]]]:
        """One best-first list of ``(user_id, score)`` per query user ID.  ``per_user_allowed_user_ids`` wins over
        ``allowed_user_ids``.  The device copy of the user-side operand is remade when that operand was edited in
        place since the copy was made."""
        self._require_n_users(recommender)
        for uid in user_ids:
            if uid not in self.user_id_to_index:
                raise RuntimeError(f"User with user_id {uid} not found.")
        rows = np.asarray([self.user_id_to_index[uid] for uid in user_ids], dtype=np.int64)
        if forbidden_user_ids is not None:
            assert len(forbidden_user_ids) == rows.size
        if per_user_allowed_user_ids is not None:
            assert len(per_user_allowed_user_ids) == rows.size
        allowed = per_user = forbidden = None
        if per_user_allowed_user_ids is not None:
            per_user = [self._known_user_indices(ids) for ids in per_user_allowed_user_ids]
        elif allowed_user_ids is not None:
            allowed = self._known_user_indices(allowed_user_ids)
        if forbidden_user_ids is not None:
            forbidden = [self._known_user_indices(ids) for ids in forbidden_user_ids]
        dev = _neighbour_recommender(recommender, rows.size, user_side=True)
        idx, score, length = dev.similar_users_arrays(rows, cutoff, allowed, per_user, forbidden, metric)
        return [[(self.user_ids[int(u)], float(s)) for u, s in zip(idx[r, :length[r]], score[r, :length[r]])]
                for r in range(idx.shape[0])]
