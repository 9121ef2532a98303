"""The AT network: GEMM and its wrappers, wavefront / persistent / batch-1 LSTM, small elementwise ops."""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .._lib import check
from ._core import LIB, PROF, _out, _p, _ptr_table, _req, _stream

_H = sys.modules[__package__]      # the package: switches and public functions are read through it at call time


# ----------------------------------------------------------------------------- AT: GEMM + LSTM cell
def gemm(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, a_strides, b_strides, out: torch.Tensor = None,
         bias: torch.Tensor = None, accumulate: bool = False, relu: bool = False) -> torch.Tensor:
    """out[M][N] = op(A)[M][K] @ op(B)[K][N] (+out) (+bias) (relu).  a_strides = (stride_m, stride_k) of op(A) in
    elements, b_strides = (stride_k, stride_n) of op(B) -- transposes are expressed through strides."""
    _req(a, "A"); _req(b, "B")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    flags = (1 if accumulate else 0) | (2 if relu else 0)
    PROF.note_flops("egz_gemm", 2.0 * M * N * K)
    check(LIB.egz_gemm(a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(bias), M, N, K, a_strides[0], a_strides[1],
                       b_strides[0], b_strides[1], N if out.dim() < 2 else out.stride(-2), flags, _stream()), "egz_gemm")
    return out


def linear_fwd(x2d: torch.Tensor, w: torch.Tensor, bias=None, relu=False, out=None, accumulate=False):
    """x2d [M][K] @ w[N][K]^T (+bias): the nn.Linear / LSTM gate projection."""
    M, K = x2d.shape
    N = w.shape[0]
    return _H.gemm(x2d, w, M, N, K, (K, 1), (1, K), out=out, bias=bias, accumulate=accumulate, relu=relu)


def matmul_nn(a2d: torch.Tensor, w: torch.Tensor):
    """a2d [M][N] @ w[N][K] -> [M][K]  (data gradient of a Linear)."""
    M, N = a2d.shape
    K = w.shape[1]
    return _H.gemm(a2d, w, M, K, N, (N, 1), (K, 1))


def matmul_tn(a2d: torch.Tensor, b2d: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False):
    """a2d[R][M]^T @ b2d[R][N] -> [M][N]  (weight gradient: dY^T X); ``out`` = an M*N destination (gradient sink)."""
    R, M = a2d.shape
    N = b2d.shape[1]
    return _H.gemm(a2d, b2d, M, N, R, (1, M), (N, 1), out=None if out is None else _out(out, (M, N), a2d.device),
                accumulate=accumulate)


def matmul_tn_batched(a_list, b_list, outs=None):
    """[a^T @ b for a, b in zip(a_list, b_list)] in ONE launch (egz_gemm_batched): every a (R, M), every b (R, N) of one shape.
    ``outs``: per product an M*N destination (a gradient sink) or None (a fresh tensor)."""
    n = len(a_list)
    R, M = a_list[0].shape
    N = b_list[0].shape[1]
    res = []
    for i in range(n):
        _req(a_list[i], "A"); _req(b_list[i], "B")
        if tuple(a_list[i].shape) != (R, M) or tuple(b_list[i].shape) != (R, N):
            raise RuntimeError("matmul_tn_batched: the products must share one shape")
        o = None if outs is None else outs[i]
        res.append(torch.empty((M, N), dtype=torch.float32, device=a_list[i].device) if o is None else _out(o, (M, N), a_list[i].device))
    PROF.note_flops("egz_gemm", 2.0 * M * N * R * n)
    check(LIB.egz_gemm_batched(_ptr_table(a_list), _ptr_table(b_list), _ptr_table(res), n, M, N, R, 1, M, N, 1, N, 0, _stream()),
          "egz_gemm_batched")
    return res


def transpose2d(x: torch.Tensor) -> torch.Tensor:
    """[R][C] -> [C][R] (LDS-tiled; W_hh -> W_hh^T for the LSTM backward)."""
    _req(x, "x")
    R, C = x.shape
    out = torch.empty((C, R), dtype=torch.float32, device=x.device)
    check(LIB.egz_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), 1, C, R, 1, _stream()), "egz_nhwc_to_nchw")
    return out


def copy_into(dst: torch.Tensor, src: torch.Tensor):
    """Stream-ordered device copy between contiguous fp32 buffers of the same size."""
    _req(dst, "dst"); _req(src, "src")
    if dst.numel() != src.numel():
        raise RuntimeError("copy_into: size mismatch")
    check(LIB.egz_copy(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "egz_copy")


# The recurrence of the AT network as ONE persistent, weight-stationary launch per direction (egz_lstm_persist_fwd / _bwd) where its
# geometry allows (L = 2, H = 512, B <= 32): T=16 / B=32 forward 167 -> 90 us, backward 190 -> 119 us (profiles/r05_ab_notes.txt).
# hipops.LSTM_PERSIST / EGAZE_LSTM_PERSIST=0: always the wavefront launches (egz_lstm_wave_fwd / _bwd: T + 1 / T + 3 launches).
# Hand-off scratch of the persistent launches: ONE buffer per (device, stream), zeroed when it is allocated and kept -- launches
# on a stream are ordered, so they may share their counters (every call zeroes those itself); its last line holds the two STICKY
# error words (forward, backward) that a timed-out hand-off raises and that no launch clears, so a failure survives the launches
# and graph replays that follow it until lstm_persist_check() looks.
_PERSIST_SYNC: dict = {}


def _persist_sync(dev: torch.device, stream_handle=None) -> torch.Tensor:
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), _stream() if stream_handle is None else stream_handle)
    buf = _PERSIST_SYNC.get(key)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            # (an allocation inside a capture would come from the graph's private pool and be zeroed by nothing)
            raise RuntimeError("persistent LSTM launch inside a hipGraph capture that did not go through hipops.capture() "
                               "(which creates the capture stream's hand-off scratch before the capture begins)")
        buf = torch.zeros((LIB.egz_lstm_persist_sync_words(),), dtype=torch.int32, device=dev)
        _PERSIST_SYNC[key] = buf
    return buf


def lstm_persist_errors() -> dict:
    """The sticky error words of every persistent-LSTM scratch (synchronises): {'fwd': e, 'bwd': e}, 0 = every in-launch hand-off
    arrived since the last reset, 1 + s = some launch had a block give up waiting in global step s (that launch's outputs -- and
    every gradient derived from them -- are NaN from that step on)."""
    out = {"fwd": 0, "bwd": 0}
    for buf in _PERSIST_SYNC.values():
        w = buf[-32:-30].tolist()
        out["fwd"] = max(out["fwd"], int(w[0]))
        out["bwd"] = max(out["bwd"], int(w[1]))
    return out


def lstm_persist_status() -> int:
    """0 when no persistent LSTM launch since the last reset lost a hand-off, else the larger of the two sticky words."""
    e = _H.lstm_persist_errors()
    return max(e["fwd"], e["bwd"])


def lstm_persist_check(reset: bool = True) -> None:
    """Raise if a persistent LSTM launch timed out since the last check.  Called where the training loops synchronise anyway (the
    AT loss-ring drain, AT.trainLSTM's per-epoch read-back).  The poisoned step did not reach the weights (FusedAdam skips
    non-finite gradient elements), so the caller can continue on the wavefront launches: the check switches the persistent form
    off for the rest of the process before it raises."""
    e = _H.lstm_persist_errors()
    if e["fwd"] or e["bwd"]:
        _H.LSTM_PERSIST = False
        if reset:
            for buf in _PERSIST_SYNC.values():
                buf[-32:].zero_()
        raise RuntimeError(f"persistent LSTM launch lost an in-launch hand-off (forward: {e['fwd']}, backward: {e['bwd']}; 1 + the "
                           f"global step a block gave up in): not every block got a compute unit -- another kernel was holding CUs "
                           f"for longer than 0.5 s.  The outputs of that step were NaN and FusedAdam skipped them; the "
                           f"persistent form is now off (wavefront launches from here on; EGAZE_LSTM_PERSIST=0 selects them "
                           f"from the start)")


class lstm_persistent:
    """``with hipops.lstm_persistent(False): ...`` -- the wavefront launches inside the block.  The persistent kernels hold one block
    per CU until the sequence is over, so they are the wrong form for an AT step that runs in the shadow of other work on the same
    device (bench.py's combined step: the SP step's MFMA kernels occupy every CU; measured +0.1 ... +0.2 ms on the SP step)."""

    def __init__(self, on: bool):
        self.on = bool(on)

    def __enter__(self):
        self.prev, _H.LSTM_PERSIST = _H.LSTM_PERSIST, self.on
        return self

    def __exit__(self, *exc):
        _H.LSTM_PERSIST = self.prev
        return False


def lstm_wave_fwd(gx0, w_ih, w_hh, bsum, h0, c0, want_acts: bool = True):
    """The stacked recurrence as a wavefront over (layer, step) (egz_lstm_wave_fwd): gx0 (T,B,4H) = layer 0's input projection
    of every step (bias included); w_ih / w_hh / bsum: lists of L tensors (w_ih[0] / bsum[0] unused); h0, c0 (L,B,H)
    -> hs_ext (L,T+1,B,H) [slot 0 of a layer = its h0, slots 1..T = the outputs], cs (L,T,B,H), acts (L,T,B,4H) | None,
    hn, cn (L,B,H)."""
    _req(gx0, "gx0"); _req(h0, "h0"); _req(c0, "c0")
    L = len(w_hh)
    T, B, H4 = gx0.shape
    Hd = H4 // 4
    for l in range(L):
        _req(w_hh[l], "w_hh")
        if l:
            _req(w_ih[l], "w_ih"); _req(bsum[l], "bias")
            if tuple(w_ih[l].shape) != (H4, Hd):
                raise RuntimeError("lstm_wave_fwd: the upper layers take the hidden size as their input size")
    dev = gx0.device
    hs = torch.empty((L, T + 1, B, Hd), dtype=torch.float32, device=dev)
    cs = torch.empty((L, T, B, Hd), dtype=torch.float32, device=dev)
    acts = torch.empty((L, T, B, H4), dtype=torch.float32, device=dev) if want_acts else None
    hn = torch.empty((L, B, Hd), dtype=torch.float32, device=dev)
    cn = torch.empty_like(hn)
    PROF.note_flops("egz_lstm_wave_fwd", 2.0 * T * B * H4 * Hd * (2 * L - 1))
    check(LIB.egz_lstm_wave_fwd(gx0.data_ptr(), _ptr_table([None] + list(w_ih[1:])), _ptr_table(w_hh),
                                _ptr_table([None] + list(bsum[1:])), h0.data_ptr(), c0.data_ptr(), hs.data_ptr(), cs.data_ptr(),
                                _p(acts), hn.data_ptr(), cn.data_ptr(), L, T, B, Hd, _stream()), "egz_lstm_wave_fwd")
    return hs, cs, acts, hn, cn


def lstm_wave_bwd(dh_top, dhn, dcn, acts, cs, c0, w_hh_t, w_ih_t):
    """Backward through time of the stack -> (dgates (L,T,B,4H), dh0 (L,B,H), dc0 (L,B,H)); w_hh_t / w_ih_t: lists of the
    transposed weights (H,4H) per layer (w_ih_t[0] unused)."""
    L, T, B, Hd = cs.shape
    dev = cs.device
    dgates = torch.empty((L, T, B, 4 * Hd), dtype=torch.float32, device=dev)
    dh0 = torch.empty((L, B, Hd), dtype=torch.float32, device=dev)
    dc0 = torch.empty_like(dh0)
    for name, t in (("dh_top", dh_top), ("dhn", dhn), ("dcn", dcn)):
        if t is not None:
            _req(t, name)
    # the gradient each lower layer receives from the layer above, formed one launch ahead of the cell backward that reads it
    dhin = torch.empty((L - 1, T, B, Hd), dtype=torch.float32, device=dev) if L > 1 else None
    PROF.note_flops("egz_lstm_wave_bwd", 2.0 * (T + 1) * B * 4 * Hd * Hd * L + 2.0 * T * B * 4 * Hd * Hd * (L - 1))
    check(LIB.egz_lstm_wave_bwd(_p(dh_top), _p(dhn), _p(dcn), acts.data_ptr(), cs.data_ptr(), c0.data_ptr(),
                                _ptr_table(w_hh_t), _ptr_table([None] + list(w_ih_t[1:])), dgates.data_ptr(), dh0.data_ptr(),
                                dc0.data_ptr(), _p(dhin), L, T, B, Hd, _stream()), "egz_lstm_wave_bwd")
    return dgates, dh0, dc0


def lstm_persist_ok(L: int, B: int, Hd: int) -> bool:
    """Whether the recurrence runs as the persistent launches (knob on and the geometry they are built for)."""
    if not (_H.LSTM_PERSIST and L == 2 and Hd == 512 and 1 <= B <= 32):
        return False
    # one block per CU, all resident at once (backward: 64 unit slices x ceil(B / 8) batch tiles)
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count >= max(128 * ((B + 15) // 16), 64 * ((B + 7) // 8))


def lstm_persist_fwd(gx0, w_ih, w_hh, b_ih, b_hh, h0, c0, want_acts: bool = True):
    """The stacked recurrence in ONE persistent, weight-stationary launch (egz_lstm_persist_fwd; L = 2, H = 512, B <= 32): gx0
    (T,B,4H) = layer 0's input projection WITHOUT bias; w_ih / w_hh / b_ih / b_hh: lists of L tensors as the module holds them
    (w_ih[0] unused) -> the outputs of lstm_wave_fwd.  The launch's hand-off counters live in a scratch of this call's own (the
    call zeroes them) and sticky error words live in this (device, stream)'s scratch (_persist_sync; lstm_persist_check())."""
    _req(gx0, "gx0"); _req(h0, "h0"); _req(c0, "c0")
    L = len(w_hh)
    T, B, H4 = gx0.shape
    Hd = H4 // 4
    for l in range(L):
        _req(w_hh[l], "w_hh"); _req(b_ih[l], "b_ih"); _req(b_hh[l], "b_hh")
        if l:
            _req(w_ih[l], "w_ih")
    dev = gx0.device
    hs = torch.empty((L, T + 1, B, Hd), dtype=torch.float32, device=dev)
    cs = torch.empty((L, T, B, Hd), dtype=torch.float32, device=dev)
    acts = torch.empty((L, T, B, H4), dtype=torch.float32, device=dev) if want_acts else None
    hn = torch.empty((L, B, Hd), dtype=torch.float32, device=dev)
    cn = torch.empty_like(hn)
    sync = _persist_sync(dev)
    PROF.note_flops("egz_lstm_persist_fwd", 2.0 * T * B * H4 * Hd * (2 * L - 1))
    check(LIB.egz_lstm_persist_fwd(gx0.data_ptr(), _ptr_table([None] + list(w_ih[1:])), _ptr_table(w_hh), _ptr_table(b_ih),
                                   _ptr_table(b_hh), h0.data_ptr(), c0.data_ptr(), hs.data_ptr(), cs.data_ptr(), _p(acts),
                                   hn.data_ptr(), cn.data_ptr(), sync.data_ptr(), L, T, B, Hd, _stream()), "egz_lstm_persist_fwd")
    return hs, cs, acts, hn, cn


def lstm_persist_bwd(dh_top, dhn, dcn, acts, cs, c0, w_hh, w_ih, db=None):
    """Backward through time in ONE persistent launch (egz_lstm_persist_bwd) -> (dgates (L,T,B,4H), dh0, dc0 (L,B,H)); w_hh / w_ih:
    the UNtransposed weights (w_ih[0] unused); db: list of 2 L destinations (b_ih_l0, b_hh_l0, b_ih_l1, b_hh_l1; None entries
    skipped) that receive the bias gradients -- the sums of dgates over steps and batch rows -- from the same launch."""
    L, T, B, Hd = cs.shape
    dev = cs.device
    dgates = torch.empty((L, T, B, 4 * Hd), dtype=torch.float32, device=dev)
    dh0 = torch.empty((L, B, Hd), dtype=torch.float32, device=dev)
    dc0 = torch.empty_like(dh0)
    for name, t in (("dh_top", dh_top), ("dhn", dhn), ("dcn", dcn)):
        if t is not None:
            _req(t, name)
    for l in range(L):
        _req(w_hh[l], "w_hh")
        if l:
            _req(w_ih[l], "w_ih")
    if db is not None:
        for t in db:
            if t is not None and (not t.is_contiguous() or t.numel() != 4 * Hd):
                raise RuntimeError("lstm_persist_bwd: a bias-gradient destination must be a contiguous (4H,) tensor")
    sync = _persist_sync(dev)
    PROF.note_flops("egz_lstm_persist_bwd", 2.0 * (T + 1) * B * 4 * Hd * Hd * L + 2.0 * T * B * 4 * Hd * Hd * (L - 1))
    check(LIB.egz_lstm_persist_bwd(_p(dh_top), _p(dhn), _p(dcn), acts.data_ptr(), cs.data_ptr(), c0.data_ptr(), _ptr_table(w_hh),
                                   _ptr_table([None] + list(w_ih[1:])), dgates.data_ptr(), dh0.data_ptr(), dc0.data_ptr(),
                                   _ptr_table(db) if db is not None else None, sync.data_ptr(), L, T, B, Hd, _stream()),
          "egz_lstm_persist_bwd")
    return dgates, dh0, dc0


def _lstm_b1_dims(params, h0, c0, what):
    """(L, C, H, N) of a 4L + 2 parameter list in state-dict order.  The C-ABI takes one (C, H, N) and strides every buffer by
    it, so a tensor of another shape would be read or written out of bounds: ValueError before anything is launched.
    (The step is launch-bound and runs once per fixation sample: the check is 4L + 4 tuple comparisons, 5 us of host time per
    call at L = 2, measured with timeit; profiles/b1_glue_tests.txt.)"""
    n = len(params)
    if n < 6 or (n - 2) % 4:
        raise ValueError(f"{what}: {n} parameters, expected 4 L + 2 (w_ih, w_hh, b_ih, b_hh per layer, lin.weight, lin.bias)")
    L = (n - 2) // 4
    if params[0].dim() != 2 or params[1].dim() != 2 or params[-2].dim() != 2:
        raise ValueError(f"{what}: w_ih_l0, w_hh_l0 and lin.weight must be matrices")
    C, Hd, N = params[0].shape[1], params[1].shape[1], params[-2].shape[0]
    want = []
    for l in range(L):
        want += [(4 * Hd, C if l == 0 else Hd), (4 * Hd, Hd), (4 * Hd,), (4 * Hd,)]
    want += [(N, Hd), (N,), (L, Hd)]
    for i, t in enumerate(params):
        if t.shape != want[i]:
            raise ValueError(f"{what}: parameter {i} has shape {tuple(t.shape)}, expected {want[i]} (L={L} C={C} H={Hd} N={N})")
    if h0.shape != want[-1] or c0.shape != want[-1]:
        raise ValueError(f"{what}: h0 {tuple(h0.shape)} / c0 {tuple(c0.shape)}, expected {(L, Hd)}")
    return L, C, Hd, N


def lstm_b1_fwd(params, inp, h0, c0, want_acts: bool = True):
    """The whole lstmnet step at T = 1, B = 1 in one call (csrc/lstm_b1.hip).  params: state-dict order, 4L + 2 tensors;
    inp (C,) raw; h0, c0 (L,H) -> (xt (C,), acts (L,4H) | None, hn (L,H), cn (L,H), out (N,))."""
    L, C, Hd, N = _lstm_b1_dims(params, h0, c0, "lstm_b1_fwd")
    for i, t in enumerate(params):
        _req(t, f"param{i}")
    _req(inp, "input"); _req(h0, "h0"); _req(c0, "c0")
    if inp.numel() != C:
        raise ValueError(f"lstm_b1_fwd: input of {inp.numel()} values, expected C = {C}")
    dev = inp.device
    xt = torch.empty(C, dtype=torch.float32, device=dev)
    acts = torch.empty((L, 4 * Hd), dtype=torch.float32, device=dev) if want_acts else None
    hc = torch.empty((2, L, Hd), dtype=torch.float32, device=dev)     # (hn, cn) in one buffer: a caller can copy both at once
    hn, cn = hc[0], hc[1]
    out = torch.empty(N, dtype=torch.float32, device=dev)
    check(LIB.egz_lstm_b1_fwd(_ptr_table(params), L, inp.data_ptr(), h0.data_ptr(), c0.data_ptr(), xt.data_ptr(), _p(acts),
                              hn.data_ptr(), cn.data_ptr(), out.data_ptr(), C, Hd, N, _stream()), "egz_lstm_b1_fwd")
    return xt, acts, hn, cn, out


def lstm_b1_bwd(params, grads, dout, dhn, dcn, xt, acts, h0, c0, hn, cn, out):
    """Backward of lstm_b1_fwd: fills the tensors in ``grads`` (same order as params; None entries are skipped)."""
    L, C, Hd, N = _lstm_b1_dims(params, h0, c0, "lstm_b1_bwd")
    for name, t in (("dout", dout), ("dhn", dhn), ("dcn", dcn)):
        if t is not None:
            _req(t, name)
    if len(grads) != len(params) or any(g is not None and g.numel() != p.numel() for g, p in zip(grads, params)):
        raise ValueError(f"lstm_b1_bwd: the gradient buffers do not match the {len(params)} parameters")
    sizes = (("dout", dout, N), ("dhn", dhn, L * Hd), ("dcn", dcn, L * Hd), ("xt", xt, C), ("acts", acts, L * 4 * Hd),
             ("hn", hn, L * Hd), ("cn", cn, L * Hd), ("out", out, N))
    for name, t, want in sizes:
        if t is not None and t.numel() != want:
            raise ValueError(f"lstm_b1_bwd: {name} holds {t.numel()} values, expected {want} (L={L} C={C} H={Hd} N={N})")
    nbytes = LIB.egz_lstm_b1_ws_bytes(L, C, Hd, N)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=out.device)
    check(LIB.egz_lstm_b1_bwd(_ptr_table(params), _ptr_table(grads), L, dout.data_ptr(), _p(dhn), _p(dcn), xt.data_ptr(),
                              acts.data_ptr(), h0.data_ptr(), c0.data_ptr(), hn.data_ptr(), cn.data_ptr(), out.data_ptr(),
                              C, Hd, N, ws.data_ptr(), nbytes, _stream()), "egz_lstm_b1_bwd")


# ----------------------------------------------------------------------------- resident LSTM vectors (data/lstm_resident.py, --lstm_resident)
LSTM_POOL_STATUS = {1: "the step cursor outside the plan", 2: "a plan row outside the pool",
                    3: "the step cursor outside the plan and a plan row outside the pool"}


def check_lstm_pool_status(word) -> None:
    """Raises if the sticky status word of lstm_pool_fetch (already read back: an int) is not 0."""
    st = int(word)
    if st:
        raise RuntimeError(f"lstm_pool_fetch: {LSTM_POOL_STATUS.get(st, st)}: the step was refused, nothing was fetched and the "
                           f"cursor did not advance")


def lstm_pool_fetch(pool: torch.Tensor, plan, cursor: torch.Tensor, inp: torch.Tensor, tgt: torch.Tensor,
                    state: Optional[torch.Tensor], status: torch.Tensor) -> None:
    """One step of the AT LSTM loops fetched on the device (egz_lstm_pool_fetch): with k = cursor[0], ``inp`` = pool[in_row[k]],
    ``tgt`` = pool[tgt_row[k]], ``state`` (optional) zeroed if reset[k], then cursor = (k + 1, k).

    pool: fp32 (F, W); plan: (in_row int32, tgt_row int32, reset uint8), each (n_steps,); cursor: int32 (2,); inp, tgt: fp32 of W
    values; state: fp32 or None; status: int32 (1,), zero-filled by the caller ONCE -- a refused step (LSTM_POOL_STATUS) ORs
    its bit in and writes nothing else; read it back where the loop synchronises and hand it to check_lstm_pool_status.  All
    tensors contiguous and on the pool's device.  The call reads nothing back, so it can be captured into a hipGraph."""
    if not (isinstance(pool, torch.Tensor) and pool.is_cuda and pool.dtype == torch.float32 and pool.dim() == 2
            and pool.is_contiguous() and pool.shape[0] >= 1 and pool.shape[1] >= 1):
        raise ValueError("lstm_pool_fetch: pool must be a contiguous float32 (F, W) tensor on the GPU")
    dev = pool.device
    F, W = pool.shape
    if W > 4096:
        raise ValueError(f"lstm_pool_fetch: W = {W}, the loss kernel of the step takes up to 4096 values")
    if not (isinstance(plan, (tuple, list)) and len(plan) == 3):
        raise ValueError("lstm_pool_fetch: plan must be (in_row, tgt_row, reset)")
    in_row, tgt_row, reset = plan
    for name, t, dt in (("in_row", in_row, torch.int32), ("tgt_row", tgt_row, torch.int32), ("reset", reset, torch.uint8)):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and t.dim() == 1 and t.is_contiguous()
                and t.numel() == in_row.numel() and t.numel() >= 1):
            raise ValueError(f"lstm_pool_fetch: {name} must be a contiguous {dt} (n_steps,) tensor on the pool's device, "
                             f"n_steps >= 1 and the same for the three plan arrays")
    if not (isinstance(cursor, torch.Tensor) and cursor.device == dev and cursor.dtype == torch.int32 and cursor.numel() == 2
            and cursor.is_contiguous()):
        raise ValueError("lstm_pool_fetch: cursor must be a contiguous int32 tensor of 2 values on the pool's device")
    for name, t in (("inp", inp), ("tgt", tgt)):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.numel() == W
                and t.is_contiguous()):
            raise ValueError(f"lstm_pool_fetch: {name} must be a contiguous float32 tensor of W = {W} values on the pool's device")
    if state is not None and not (isinstance(state, torch.Tensor) and state.device == dev and state.dtype == torch.float32
                                  and state.is_contiguous()):
        raise ValueError("lstm_pool_fetch: state must be None or a contiguous float32 tensor on the pool's device")
    if not (isinstance(status, torch.Tensor) and status.device == dev and status.dtype == torch.int32 and status.numel() == 1):
        raise ValueError("lstm_pool_fetch: status must be an int32 tensor of 1 value on the pool's device")
    check(LIB.egz_lstm_pool_fetch(pool.data_ptr(), F, W, in_row.data_ptr(), tgt_row.data_ptr(), reset.data_ptr(),
                                  in_row.numel(), cursor.data_ptr(), inp.data_ptr(), tgt.data_ptr(), _p(state),
                                  0 if state is None else state.numel(), status.data_ptr(), _stream()), "egz_lstm_pool_fetch")


def lstm_cell_fwd(gates, c_prev, h_out, c_out, act):
    B, Hd = c_prev.shape
    check(LIB.egz_lstm_cell_fwd(gates.data_ptr(), c_prev.data_ptr(), h_out.data_ptr(), c_out.data_ptr(), _p(act), B, Hd,
                                _stream()), "egz_lstm_cell_fwd")


def lstm_cell_bwd(act, c, c_prev, dh, dc_in, dgates, dc_prev):
    B, Hd = c.shape
    check(LIB.egz_lstm_cell_bwd(act.data_ptr(), c.data_ptr(), c_prev.data_ptr(), dh.data_ptr(), _p(dc_in),
                                dgates.data_ptr(), dc_prev.data_ptr(), B, Hd, _stream()), "egz_lstm_cell_bwd")


def tanh_fwd(x):
    _req(x, "x")
    y = torch.empty_like(x)
    check(LIB.egz_tanh_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "egz_tanh_fwd")
    return y


def tanh_bwd(y, dy):
    dx = torch.empty_like(y)
    check(LIB.egz_tanh_bwd(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.numel(), _stream()), "egz_tanh_bwd")
    return dx


def add(a, b):
    _req(a, "a"); _req(b, "b")
    out = torch.empty_like(a)
    check(LIB.egz_add(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "egz_add")
    return out
