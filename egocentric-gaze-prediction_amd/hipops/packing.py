"""Packed 3x3 weights: the cache that follows a parameter's identity, and its batched rebuild."""
from __future__ import annotations

import sys
import weakref

import torch

from .._lib import check
from ._core import LIB, _req, _stream

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- packed weights
_WEIGHT_EPOCH = [0]
_PACKED = {}
_USED = set()                     # packings requested by a launch since their last rebuild (refresh_packings)


def bump_weight_epoch():
    """Invalidate every packing (parameters were overwritten wholesale behind torch's back, e.g. a DP broadcast).
    The blunt half of the rule for writes torch cannot see ("Writes behind torch's back"): every packed
    weight, BatchNorm fold and eval row of every model is rebuilt at its next use, and a captured step repacks."""
    _WEIGHT_EPOCH[0] += 1


def touch_params(params):
    """Called by the fused optimizer after it rewrote THESE parameters through its flat buffer (no torch version bump):
    only their packings go stale -- a second optimizer (the AT module's) must not invalidate the SP model's.
    Also what a caller owes after writing a parameter or a BatchNorm buffer through ``.data``, ``dist.broadcast(p.data)`` or a
    raw pointer ("Writes behind torch's back"): such a write moves neither the version counter nor the
    address, so nothing else can see it."""
    for p in params:
        p._egz_epoch = getattr(p, "_egz_epoch", 0) + 1
    log = _CAPTURE_LOG[0]
    if log is not None:             # inside hipops.capture(): every replay of the graph writes these again (note_replay)
        log[0].extend(params)


# While ``hipops.capture()`` is open: [tensors declared written (touch_params: FusedAdam.step, bn_finalize*), keys of the packings
# the captured launches rebuild (refresh_packings)].  The host side of a captured step runs once; its kernels run on every replay.
_CAPTURE_LOG = [None]


def note_replay(written, rebuilt):
    """After ``graph.replay()`` of a capture that logged ``written`` / ``rebuilt`` (``hipops.capture.written`` / ``.rebuilt``):
    declare the replay's device-side writes the way the eager step does (the per-tensor epoch: eval rows, BatchNorm folds, eval-only
    packing kinds and graphs.GraphedModule go stale), and stamp the packings the replay itself rebuilt AFTER those writes with the
    new tag (they are fresh).  Host only: no launch, no synchronisation."""
    for p in written:
        p._egz_epoch = getattr(p, "_egz_epoch", 0) + 1
    for key in rebuilt:
        hit = _PACKED.get(key)
        w = hit[2]() if hit is not None else None
        if w is not None:
            _PACKED[key] = (_tag(w), hit[1], hit[2])


def _tag(w):
    return (_WEIGHT_EPOCH[0], getattr(w, "_egz_epoch", 0), w._version, w.data_ptr())


_UID = [0]


def _uid(w: torch.Tensor) -> int:
    """Identity of a weight tensor that cannot be recycled the way a data_ptr can: a counter stored on the
    tensor object (torch preserves the Python object of a live tensor); the cache entry dies with the tensor."""
    uid = getattr(w, "_egz_uid", None)
    if uid is None:
        _UID[0] += 1
        uid = _UID[0]
        w._egz_uid = uid
        weakref.finalize(w, _drop_packed, uid)
    return uid


_PACK_FN = {"fwd": ("egz_pack_w3x3_fwd", 0, 0), "dgrad": ("egz_pack_w3x3_dgrad", 0, 1),
            "ups_fwd": ("egz_pack_w3x3_ups_fwd", 1, 2), "ups_dgrad": ("egz_pack_w3x3_ups_dgrad", 1, 3),
            # MFMA-fragment-ordered split packings of the streamed-weight kernel (split dtypes only)
            "fwd_frag": (None, 0, 4), "dgrad_frag": (None, 0, 5), "ups_dgrad_frag": (None, 1, 6),
            "ups_fwd_frag": (None, 1, 7)}


def _drop_packed(uid: int):
    for kind in _PACK_FN:
        for dt in (0, 1, 2):
            _PACKED.pop((uid, kind, dt), None)


def packed_weight(w: torch.Tensor, kind: str, dtype: int = 0) -> torch.Tensor:
    """(Cout, Cin, [1,] 3, 3) -> the kernels' private packed layout: 'fwd' / 'dgrad' (9 taps) or, for a conv that
    follows a nearest x2 upsample, 'ups_fwd' (4 phases x 2x2 pre-summed taps) / 'ups_dgrad' (4x4 stride-2 taps).
    Pass the parameter object itself (not a detached alias) so the cache can follow its identity."""
    _req(w, "weight")
    K, C = w.shape[0], w.shape[1]
    key = (_uid(w), kind, dtype)
    tag = _tag(w)
    hit = _PACKED.get(key)
    if hit is not None and hit[0] == tag:
        _USED.add(key)
        return hit[1]
    fname, ekind, kidx = _PACK_FN[kind]
    buf = hit[1] if hit is not None else torch.empty(LIB.egz_pack_w3x3_elems(C, K, ekind), dtype=torch.float32,
                                                     device=w.device)
    if kidx >= 4:
        if not dtype:
            raise RuntimeError("fragment-ordered packings exist for the split-half dtypes only")
        check(LIB.egz_pack_w3x3_split_frag(w.data_ptr(), buf.data_ptr(), C, K, kidx, dtype, _stream()),
              "egz_pack_w3x3_split_frag")
    elif dtype:      # hi / lo 16-bit planes (same byte count as the fp32 packing)
        check(LIB.egz_pack_w3x3_split(w.data_ptr(), buf.data_ptr(), C, K, kidx, dtype, _stream()), "egz_pack_w3x3_split")
    else:
        check(getattr(LIB, fname)(w.data_ptr(), buf.data_ptr(), C, K, _stream()), fname)
    _PACKED[key] = (tag, buf, weakref.ref(w))
    _USED.add(key)
    return buf


# hipops.BATCH_REPACK: FusedAdam.step() rebuilds the stale fragment-ordered packings of its parameters in ONE launch (False:
# each packing is rebuilt lazily in front of the first launch that needs it; test_pack_frag_batch_matches_per_layer flips it)
_BATCH_TABLES = {}
_BATCH_PINNED = set()          # tables whose launch was captured into a hipGraph: never evicted


def refresh_packings(params, force: bool = False) -> int:
    """Rebuild, in one launch on the current stream, every fragment-ordered split packing of ``params`` that went stale and
    that some launch has used since its last rebuild (egz_pack_w3x3_frag_batch; bit-identical to the lazy per-layer rebuilds).
    Returns the number of packings rebuilt.  Packings nobody asked for since the last rebuild (eval-only kinds, a layer whose
    geometry changed) stay stale and are rebuilt lazily by packed_weight().  ``force``: every existing fragment-ordered packing
    of ``params``, stale by its tag or not (a captured training step whose parameters were overwritten between two replays)."""
    if not _H.BATCH_REPACK or not (_USED or force):
        return 0
    ids = {getattr(p, "_egz_uid", None) for p in params}
    todo = []
    for key in sorted(k for k in (_PACKED if force else _USED) if k[0] in ids and k[2] and _PACK_FN[k[1]][2] >= 4):
        hit = _PACKED.get(key)
        w = hit[2]() if hit is not None else None
        if w is None:
            _USED.discard(key)
            continue
        if force or hit[0] != _tag(w):
            todo.append((key, w, hit[1]))
    if not todo:
        return 0
    sig = tuple((key, w.data_ptr(), buf.data_ptr()) for key, w, buf in todo)
    ent = _BATCH_TABLES.get(sig)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is None and capturing:
        # No table for THIS set inside a hipGraph capture (the warm-up step before the capture touched another set: an eval
        # pass in between, a table eviction): building one needs a host -> device copy, which a capture cannot hold.  The
        # per-key pack launches need no table and are capturable -- the captured step then repacks exactly this set on every
        # replay (returning 0 here left every replay after the first on stale packed weights).
        for key, w, buf in todo:
            check(LIB.egz_pack_w3x3_split_frag(w.data_ptr(), buf.data_ptr(), w.shape[1], w.shape[0], _PACK_FN[key[1]][2], key[2],
                                               _stream()), "egz_pack_w3x3_split_frag")
    else:
        if ent is None:
            rows, nb = [], 0
            for key, w, buf in todo:
                K, C = w.shape[0], w.shape[1]
                rows.append([w.data_ptr(), buf.data_ptr(), C, K, _PACK_FN[key[1]][2], key[2], nb, 0])
                nb += LIB.egz_pack_w3x3_frag_blocks(C, K)
            if len(_BATCH_TABLES) > 64:
                # (a table a captured graph replays from must stay alive: its launch baked the table's address in)
                for k_ in [k_ for k_ in _BATCH_TABLES if k_ not in _BATCH_PINNED]:
                    del _BATCH_TABLES[k_]
            ent = (torch.tensor(rows, dtype=torch.int64).to(todo[0][1].device), nb)
            _BATCH_TABLES[sig] = ent
        if capturing:
            _BATCH_PINNED.add(sig)
        check(LIB.egz_pack_w3x3_frag_batch(ent[0].data_ptr(), len(todo), ent[1], _stream()), "egz_pack_w3x3_frag_batch")
    log = _CAPTURE_LOG[0]
    for key, w, buf in todo:
        _PACKED[key] = (_tag(w), buf, weakref.ref(w))
        _USED.discard(key)
        if capturing and log is not None:
            log[1].append(key)
    return len(todo)


def repack_stale(params) -> int:
    """Rebuild now, on the current stream and into their existing buffers, every packing of ``params`` (any kind) whose tag went
    stale: a captured hipGraph bakes the packed buffers in as pointers, so parameters overwritten from outside between two replays
    (``load_state_dict`` into a frozen encoder) must be repacked before the next replay.  Returns the number of packings rebuilt."""
    ids = {getattr(p, "_egz_uid", None) for p in params}
    n = 0
    for key in [k for k in _PACKED if k[0] in ids]:
        hit = _PACKED.get(key)
        w = hit[2]() if hit is not None else None
        if w is not None and hit[0] != _tag(w):
            _H.packed_weight(w, key[1], key[2])
            n += 1
    return n
