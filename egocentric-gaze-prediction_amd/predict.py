"""Gaze prediction on an unlabelled video: frames in, gaze track out, everything between on the GPU.

    python -m egaze_amd.predict --framePath VIDEO_FOLDER --trained_model best_SP.pth.tar --trained_late best_late.pth.tar
        [--trained_lstm best_lstm.pth.tar] --out DIR [--fixsac all|auto|FILE] [--fix_radius 17.5] [--chunk 32] [--crop_size 3]
        [--flow_jpeg 95] [--handover_jpeg 0] [--overlay] [--save_maps] [--device 0] [TV-L1 options and --bound as extract_flow]

The full model (SP -> AT -> LF) as the three training drivers run it, without a ground-truth map, a file between the stages or a
host round trip per frame.  ``VIDEO_FOLDER`` holds the frames of ONE video as ``img_%05d.jpg``; frames that are not 224 x 224 are
resized as ``extract_flow --size 224 224`` resizes them and the outputs are mapped back to the original size.

Frames and flows.  With F frames indexed 0 .. F - 1, flow i goes from frame i to frame i + 1 (extract_flow's numbering).  Frame k
gets a prediction iff 9 <= k <= F - 2: its flow stack is STdatas.build_temporal_list's -- channel 2m the x-flow k - m, channel
2m + 1 the y-flow k - m, m = 0 .. 9.  F < 11 is refused.  Every flow is computed once: a chunk hands its last frame (BGR and grey)
and its last nine flow pairs to the next.  With ``--flow_jpeg Q`` (default 95, extract_flow's) the flow images go through
hipops.jpeg_roundtrip(Q) -- the planes jpeg_decode gives for jpeg_encode(Q)'s files, bit for bit, without the bitstream -- so
that the temporal stream sees the bytes it was trained on; 0 skips that.

Per chunk of n <= ``--chunk`` predictable frames (VideoPredictor._launch): the chunk's BGR planes and its n + 9 flow pairs sit in
one uint8 pool, a host-built (n, 22) plane table (column 21 = -1: no ground truth) drives ONE resident_gather launch, then
  1 SP eval forward -> out (n,1,224,224), features_s (n,512,14,14);
  2 com_sp, gp, q_sp = u8_center_of_mass(out): the gaze point is the PREDICTED one, floor(com_sp), as in run_spatialstream
    (AT.extract_late takes the ground-truth arg-max there);
  3 rows = crop_mean(features_s, gp, crop_size, 16);
  4 the fixation flags (below);
  5 the saccade frames of the chunk (flag != 1), in order, are ONE lstmnet call at batch 1, state carried across chunks from
    None (AT.extract_late's chain); their outputs replace their rows;
  6 at = weighted_minmax(features_s, rows); fused, planes = late_input(q_sp, at): the hand-over extract_late writes and
    lateDataset reads, on the device; ``--handover_jpeg Q`` sends both planes through jpeg_roundtrip(Q) first (for an LF
    trained from .jpg-named hand-over files);
  7 fin = late.fusion(fused) (eval mode, as run_spatialstream runs it); com, _, q_fin = u8_center_of_mass(fin).
One read-back per chunk (com, com_sp and the status words, waited for a chunk later); ``auto`` needs com_sp on the host before
step 5 and costs a second one.  ``--flow_jpeg`` / ``--handover_jpeg`` add no wait: the round trip is one launch whose status
words come back with the chunk's.  jpeg_encode reads the lengths of its files back, once per call: with ``--overlay`` /
``--save_maps`` each encode adds that wait.  File writes are host I/O and run a chunk behind.

Fixation flags (``--fixsac``).  ``all`` (default): every frame is a fixation -- the reference README's stated assumption for its
simple test; the LSTM is never loaded or called.  FILE: one float per frame of the video, line k for frame k, dilated as
STDataset dilates its labels.  ``auto``: the dispersion rule of misc/gazedataset_gt.py (fixation_state) run ONLINE on com_sp in
224-map pixels with squared radius fix_radius^2 (17.5 = the reference's 50 px of 640 scaled to 224), without the rule's
retroactive un-marking of one-frame fixations; the first predictable frame counts as a saccade.  ``auto`` is a STAND-IN with an
untuned threshold, NOT the paper's fixation predictor: the reference ships none and its README invites "any method".

Outputs.  ``gaze.csv``: frame,row,col,x,y,fixation,sp_row,sp_col per predictable frame -- frame = the number in the file name,
(row, col) = com in 224-map pixels, x = (col + 0.5) W0 / 224 - 0.5 and y = (row + 0.5) H0 / 224 - 0.5 in original-frame pixels,
(sp_row, sp_col) = com_sp.  An all-zero final map has no centre of mass: empty coordinates and a warning.  ``--save_maps``:
q_fin as ``pred_<frame file name>`` (grey JPEG, quality 95).  ``--overlay``: ``gaze_<stem>.jpg`` at the original size --
heatmap_overlay(q_fin, frames, jet_lut), draw_ring at rint(y, x) with radii rint(6 H0 / 224) / rint(9 H0 / 224) in white, jpeg_encode."""
import argparse
import os
import time
import warnings

import numpy as np

MAP = 224                     # the network's input and map size
STACK = 10                    # flow pairs per sample
LEAD = STACK - 1              # flows a sample needs before its own: the first predictable frame
CSV_HEADER = "frame,row,col,x,y,fixation,sp_row,sp_col"
RING = (6, 9)                 # marker radii in 224-map pixels
OVERLAY_QUALITY = MAP_QUALITY = 95


# ----------------------------------------------------------------------------- host logic (no device)
def predictable_frames(nframes):
    """range of the frame indices that get a prediction: 9 <= k <= F - 2.  F < 11 raises ValueError."""
    if nframes < STACK + 1:
        raise ValueError(f"{nframes} frames: a prediction needs the ten flows that end at a frame and the flow that starts "
                         f"there, i.e. at least {STACK + 1} frames")
    return range(LEAD, nframes - 1)


def chunk_plan(nframes, chunk):
    """-> [dict] per chunk: 'frames' (k0, k1) the predictable frames [k0, k1); 'decode' (d0, d1) the frame indices [d0, d1) read
    and decoded in this chunk; 'flows' (f0, f1) the flows [f0, f1) computed in it; 'carried' (c0, c1) the flows [c0, c1) taken
    over from the chunk before.  The pool of a chunk holds flows k0 - 9 .. k1 - 1 = carried + computed; no flow and no frame
    appears in two chunks' 'flows' / 'decode'."""
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    pr = predictable_frames(nframes)
    out = []
    for k0 in range(pr.start, pr.stop, chunk):
        k1 = min(k0 + chunk, pr.stop)
        first = k0 == pr.start
        out.append({'frames': (k0, k1), 'decode': (0 if first else k0 + 1, k1 + 1), 'flows': (0 if first else k0, k1),
                    'carried': (k0 - LEAD, k0 - LEAD if first else k0)})
    return out


def plane_table(n):
    """The (n, 22) int64 plane table of a chunk of n frames (resident_gather's): the pool holds the 3 n BGR planes of the frames,
    then the x and y planes of the n + 9 flows k0 - 9 .. k1 - 1, pair by pair.  Column 0: the first BGR plane of frame i; columns
    1 + 2m / 2 + 2m: the x / y plane of flow k - m, pool pair i + 9 - m; column 21: -1 (no ground truth)."""
    t = np.full((n, 22), -1, dtype=np.int64)
    base = 3 * n
    for i in range(n):
        t[i, 0] = 3 * i
        for m in range(STACK):
            t[i, 1 + 2 * m] = base + 2 * (i + LEAD - m)
            t[i, 2 + 2 * m] = base + 2 * (i + LEAD - m) + 1
    return t


def dilate_fixsac(a):
    """STDataset.__init__'s dilation of the fixation labels by one frame each side."""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    return (np.convolve(a, np.array([1, 1, 1]))[1:-1] > 0).astype(float)


def load_fixsac(path, nframes):
    """One float per frame, line k for frame k -> the dilated flags of the first ``nframes`` lines; a shorter file is refused."""
    a = np.atleast_1d(np.loadtxt(path))
    if a.ndim != 1 or a.shape[0] < nframes:
        raise ValueError(f"{path}: {a.shape[0] if a.ndim == 1 else a.shape} fixation flags for {nframes} frames")
    return dilate_fixsac(a)[:nframes]


class OnlineFixation:
    """misc/gazedataset_gt.fixation_state fed one point at a time: a point closer than ``radius`` (squared distance < radius^2)
    to the running centre of the current fixation is a fixation sample (1) and moves the centre, the running mean in the
    reference's operation order; any other point (a NaN included) is a saccade sample (0) and becomes the new centre.  The first
    point is a saccade sample.  The reference's retroactive clearing of a one-sample fixation is left out: a frame's flag has
    been used by the time the next frame is seen.  A stand-in with an untuned threshold, not the paper's fixation predictor."""

    def __init__(self, radius=17.5):
        self.r2 = float(radius) ** 2
        self.center = None
        self.fix_num = 0

    def step(self, x, y):
        x, y = float(x), float(y)
        if self.center is not None and (self.center[0] - x) ** 2 + (self.center[1] - y) ** 2 < self.r2:
            n = self.fix_num = self.fix_num + 1
            self.center = ((self.center[0] * n + x) / (n + 1), (self.center[1] * n + y) / (n + 1))
            return 1
        self.fix_num = 0
        self.center = (x, y)
        return 0


def map_to_frame(row, col, frame_hw):
    """(row, col) in 224-map pixels -> (x, y) in pixels of an H0 x W0 frame: pixel centres map to pixel centres."""
    H0, W0 = frame_hw
    return (col + 0.5) * W0 / MAP - 0.5, (row + 0.5) * H0 / MAP - 0.5


def ring_radii(frame_h):
    """The marker's radii at an H0-high frame: rint(6 H0 / 224), rint(9 H0 / 224), the outer one at least 1."""
    r_in, r_out = (int(np.rint(r * frame_h / MAP)) for r in RING)
    return r_in, max(r_out, r_in, 1)


def build_parser():
    p = argparse.ArgumentParser(prog="egaze_amd.predict", description="gaze prediction on the frames of one video (SP -> AT -> LF)")
    a = p.add_argument
    a('--framePath', required=True, help="folder holding the img_%%05d.jpg frames of one video")
    a('--trained_model', required=True, help="SP checkpoint (best_SP.pth.tar)")
    a('--trained_late', required=True, help="LF checkpoint (best_late.pth.tar)")
    a('--trained_lstm', default=None, help="AT LSTM checkpoint (best_lstm.pth.tar); needed by --fixsac auto / FILE")
    a('--out', required=True, help="output folder: gaze.csv, pred_*.jpg (--save_maps), gaze_*.jpg (--overlay)")
    a('--fixsac', default='all', help="'all': every frame is a fixation (default); 'auto': online dispersion rule on the SP "
                                      "gaze point (a stand-in, untuned); or a file of one flag per frame")
    a('--fix_radius', type=float, default=17.5, help="--fixsac auto: dispersion radius in 224-map pixels")
    a('--chunk', type=int, default=32, help="predictable frames per GPU batch")
    a('--crop_size', type=int, default=3, help="crop of the conv5_3 map around the gaze point (AT)")
    a('--flow_jpeg', type=int, default=95, help="JPEG quality the flow images pass through (extract_flow's default); 0: none")
    a('--handover_jpeg', type=int, default=0, help="JPEG quality the SP / AT planes pass through before LF; 0: none (PNG hand-over)")
    a('--overlay', action='store_true', help="write gaze_*.jpg: heatmap and gaze marker over the original frame")
    a('--save_maps', action='store_true', help="write pred_*: the final 224 x 224 gaze map")
    a('--device', default='0', help="GPU index")
    a('--bound', type=float, default=20.0, help="flow of +-bound pixels maps to 255 / 0")
    for name, default in (('tau', 0.25), ('lam', 0.15), ('theta', 0.3), ('zfactor', 0.5)):
        a('--' + name, type=float, default=default, help=f"TV-L1 parameter (default {default})")
    for name, default in (('nscales', 5), ('warps', 5), ('iterations', 30)):
        a('--' + name, type=int, default=default, help=f"TV-L1 parameter (default {default})")
    return p


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.chunk < 1:
        parser.error("--chunk must be at least 1")
    for name in ('flow_jpeg', 'handover_jpeg'):
        if not 0 <= getattr(args, name) <= 100:
            parser.error(f"--{name} must be 0 (off) or a JPEG quality 1 .. 100")
    if not args.fix_radius >= 0:
        parser.error("--fix_radius must not be negative")
    if args.crop_size < 1:
        parser.error("--crop_size must be at least 1")
    if not args.bound > 0:
        parser.error("--bound must be positive")
    if args.fixsac != 'all' and args.trained_lstm is None:
        parser.error(f"--fixsac {args.fixsac} runs the saccade frames through the LSTM: --trained_lstm is needed")
    args.params = {k: getattr(args, k) for k in ('tau', 'lam', 'theta', 'nscales', 'zfactor', 'warps', 'iterations')}
    return args


# ----------------------------------------------------------------------------- the predictor
class _Pending:
    """A queued chunk: what the host reads once its event has passed."""

    def __init__(self):
        self.recs, self.host, self.done, self.status, self.files, self.codec = [], None, None, {}, [], []


class VideoPredictor:
    """``VideoPredictor(model, lstm, late, ...).run(frames)`` -> one record (dict) per predictable frame, in frame order:
    'index' k, 'frame' (the number in the name), 'name', 'row', 'col', 'x', 'y' (None where the final map is all zero),
    'fixation', 'sp_row', 'sp_col'; with ``keep=True`` also the frame's device tensors 'image', 'flow' (what model_SP was
    handed), 'out', 'at', 'fused', 'fin', 'q_fin'.

    model: a model_SP, lstm: an lstmnet or None (mode 'all' never calls it), late: a late_fusion -- on one GPU; all are put in
    eval mode.  fixsac: 'all', 'auto' or the path of a flag file.  ``out``: a folder for gaze.csv and, with save_maps / overlay,
    the images; None writes nothing.  ``frames``: the folder of a video or a list of its frame files in order.  ``profile``: an
    optional dict phase -> seconds (each phase then waits for the device: tools/bench_predict.py)."""

    def __init__(self, model, lstm, late, fixsac='all', fix_radius=17.5, chunk=32, crop_size=3, flow_jpeg=95, handover_jpeg=0,
                 bound=20.0, flow_params=None, overlay=False, save_maps=False, out=None, keep=False, profile=None):
        import torch
        if fixsac != 'all' and lstm is None:
            raise ValueError(f"fixsac={fixsac!r} runs the saccade frames through the LSTM: lstm is None")
        if chunk < 1:
            raise ValueError(f"chunk must be at least 1, got {chunk}")
        if (overlay or save_maps) and out is None:
            raise ValueError("overlay / save_maps need an output folder (out=)")
        self.model, self.lstm, self.late = model.eval(), (lstm.eval() if lstm is not None else None), late.eval()
        self.device = next(model.parameters()).device
        if self.device.type != 'cuda':
            raise RuntimeError("VideoPredictor: the models must be on a HIP ('cuda') device -- this package has no CPU path")
        self.fixsac, self.fix_radius, self.chunk, self.crop_size = fixsac, float(fix_radius), int(chunk), int(crop_size)
        self.flow_jpeg, self.handover_jpeg, self.bound = int(flow_jpeg), int(handover_jpeg), float(bound)
        self.flow_params = dict(flow_params or {})
        self.overlay, self.save_maps, self.out, self.keep, self.profile = overlay, save_maps, out, keep, profile
        self._feat = []
        self._hook = model.features_s.register_forward_hook(lambda mod, inp, outp: self._feat.append(outp))
        self._torch = torch

    def close(self):
        self._hook.remove()

    # ---- helpers
    def _mark(self, name, t0):
        if self.profile is not None:
            self._torch.cuda.synchronize(self.device)
            self.profile[name] = self.profile.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    def _jpeg_round_trip(self, planes, quality):
        """(N, H, W) uint8 -> the planes jpeg_decode gives for jpeg_encode(quality)'s files, bit for bit, without the files:
        one jpeg_roundtrip launch, no read-back of file lengths (profiles/flow_handover.txt has the comparison)."""
        from . import hipops as H
        dec, status = H.jpeg_roundtrip(planes.contiguous(), quality)
        self._codec.append((status, None))
        return dec

    # ---- one chunk, queued
    def _launch(self, plan, files, state, flags_file):
        torch = self._torch
        from . import hipops as H
        from .data.extract_flow import decode_frames
        from .functions import to_nhwc
        from .utils import repackage_hidden
        dev = self.device
        (k0, k1), (d0, d1) = plan['frames'], plan['decode']
        n = k1 - k0
        pend = _Pending()
        self._codec = []

        t0 = time.perf_counter()
        orig = decode_frames([files[i][1] for i in range(d0, d1)], None, dev)              # (d1 - d0, 3, H0, W0)
        if state['hw'] is None:
            state['hw'] = tuple(orig.shape[2:])
        elif tuple(orig.shape[2:]) != state['hw']:
            raise SystemExit(f"{files[d0][1]}: frames of {tuple(orig.shape[2:])}, the video began with {state['hw']}")
        small = orig if state['hw'] == (MAP, MAP) else H.resize_linear_u8(orig, (MAP, MAP), layout='chw')
        t0 = self._mark("decode", t0)

        gray = H.bgr_to_gray_u8(small)
        if state['gray'] is not None:
            gray = torch.cat((state['gray'], gray))
            bgr = torch.cat((state['bgr'], small))
            orig_all = torch.cat((state['orig'], orig)) if self.overlay else None
        else:
            bgr, orig_all = small, (orig if self.overlay else None)
        u1, u2 = H.tvl1_flow(gray, **self.flow_params)
        new = H.flow_to_u8(torch.stack((u1, u2), 1), self.bound)                            # (flows, 2, 224, 224): x, y per flow
        if self.flow_jpeg:
            new = self._jpeg_round_trip(new.view(-1, MAP, MAP), self.flow_jpeg).view(-1, 2, MAP, MAP)
        flows = new if state['flows'] is None else torch.cat((state['flows'], new))         # flows k0 - 9 .. k1 - 1
        assert flows.shape[0] == n + LEAD and bgr.shape[0] >= n + 1
        first = bgr.shape[0] - (n + 1)                    # frame k0's position: 9 in the first chunk, 0 afterwards
        state['gray'], state['bgr'], state['flows'] = gray[-1:], bgr[-1:], flows[-LEAD:]
        if self.overlay:
            state['orig'] = orig_all[-1:]
        t0 = self._mark("flow", t0)

        pool = torch.cat((bgr[first:first + n].reshape(-1, MAP, MAP), flows.reshape(-1, MAP, MAP)))
        table = torch.from_numpy(plane_table(n)).to(dev)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        image, flow, _ = H.resident_gather(pool, table, idx, fields=('image', 'flow'), status_to=pend.status)
        t0 = self._mark("gather", t0)

        del self._feat[:]
        out = self.model(image, flow)                                                       # 1
        feature = self._feat[0]
        del self._feat[:]
        t0 = self._mark("sp", t0)

        com_sp, gp, q_sp = H.u8_center_of_mass(out.reshape(n, MAP, MAP), want_u8=True)      # 2
        fn = to_nhwc(feature)
        rows = H.crop_mean(fn, gp, self.crop_size, 16)                                      # 3
        if self.fixsac == 'all':                                                            # 4
            flags = [1] * n
        elif self.fixsac == 'auto':
            pts = com_sp.cpu().numpy()                                                      # (the second read-back)
            flags = [state['auto'].step(pts[i, 1], pts[i, 0]) for i in range(n)]
        else:
            flags = [int(flags_file[k]) for k in range(k0, k1)]
        sacc = [i for i, f in enumerate(flags) if f != 1]                                   # 5
        if sacc:
            sel = torch.tensor(sacc, device=dev)
            state['hidden'] = repackage_hidden(state['hidden'])
            seq, state['hidden'] = self.lstm(rows.index_select(0, sel).unsqueeze(1), state['hidden'])
            rows = rows.index_copy(0, sel, seq.squeeze(1))
        at = H.weighted_minmax(fn, rows)                                                    # 6
        fused, planes = H.late_input(q_sp, at, want_u8=True, status_to=pend.status)
        if self.handover_jpeg:
            dec = self._jpeg_round_trip(planes.view(-1, MAP, MAP), self.handover_jpeg).view(n, 2, MAP, MAP)
            fused = H.late_input(dec[:, 1].contiguous(), dec[:, 0].contiguous(), status_to={})     # (bytes: nothing to flag)
        t0 = self._mark("glue", t0)

        fin = self.late.fusion(fused, fuse_sigmoid=True)                                    # 7
        com, _, q_fin = H.u8_center_of_mass(fin.reshape(n, MAP, MAP), want_u8=True)
        t0 = self._mark("lf", t0)

        pend.host = torch.empty((n, 4), dtype=torch.float64).pin_memory()
        pend.host.copy_(torch.cat((com, com_sp), 1), non_blocking=True)                     # the chunk's read-back
        H0, W0 = state['hw']
        if self.save_maps:
            pend.files.append(('pred_%s', self._encode(q_fin)))
        if self.overlay:
            over = H.heatmap_overlay(q_fin, orig_all, list(range(first, first + n)), H.jet_lut(dev))
            x, y = map_to_frame(com[:, 0], com[:, 1], (H0, W0))
            centers = torch.stack((torch.round(y), torch.round(x)), 1)
            centers = torch.where(torch.isnan(centers), torch.full_like(centers, -1e6), centers).to(torch.int32).contiguous()
            r_in, r_out = ring_radii(H0)
            H.draw_ring(over, centers, r_in, r_out, (255, 255, 255))
            pend.files.append(('gaze_%s', self._encode(over)))
        pend.codec = self._codec
        pend.done = torch.cuda.Event()
        pend.done.record()
        for i in range(n):
            number, path = files[k0 + i]
            rec = {'index': k0 + i, 'frame': number, 'name': os.path.basename(path), 'fixation': int(flags[i])}
            if self.keep:
                rec.update(image=image[i], flow=flow[i], out=out[i], at=at[i], fused=fused[i], fin=fin[i], q_fin=q_fin[i])
            pend.recs.append(rec)
        self._mark("encode_write", t0)
        return pend

    def _encode(self, images):
        """uint8 images on the device -> (pinned host bytes, offsets list): the files of a chunk, copied asynchronously."""
        torch = self._torch
        from . import hipops as H
        data, offsets, status = H.jpeg_encode(images, quality=MAP_QUALITY if images.dim() == 3 else OVERLAY_QUALITY)
        self._codec.append((status, None))
        host = torch.empty(data.shape, dtype=torch.uint8).pin_memory()
        host.copy_(data, non_blocking=True)
        return host, offsets.cpu().tolist()

    # ---- a queued chunk, handed over (host I/O)
    def _finish(self, pend, state, csv):
        from . import hipops as H
        t0 = time.perf_counter()
        pend.done.synchronize()
        H.check_resident_status(pend.status.pop('_resident_status'))
        H.late_input_status(pend.status.pop('_late_input_status'))      # a NaN AT map (constant features) is legitimate: 0
        for enc, dec in pend.codec:
            if int(enc.abs().max()) or (dec is not None and int(dec.abs().max())):
                raise RuntimeError(f"jpeg round trip failed: encode status {sorted(set(enc.tolist()))}, decode status "
                                   f"{sorted(set(dec.tolist())) if dec is not None else '-'}")
        vals = pend.host.numpy()
        for i, rec in enumerate(pend.recs):
            row, col, sp_row, sp_col = (float(v) for v in vals[i])
            rec['sp_row'], rec['sp_col'] = sp_row, sp_col
            if np.isnan(row) or np.isnan(col):
                warnings.warn(f"{rec['name']}: the final gaze map is all zero: no gaze point", RuntimeWarning)
                rec['row'] = rec['col'] = rec['x'] = rec['y'] = None
            else:
                rec['row'], rec['col'] = row, col
                rec['x'], rec['y'] = map_to_frame(row, col, state['hw'])
            if csv is not None:
                f = lambda v: '' if v is None or (isinstance(v, float) and np.isnan(v)) else repr(v)
                csv.write(','.join([str(rec['frame']), f(rec['row']), f(rec['col']), f(rec['x']), f(rec['y']),
                                    str(rec['fixation']), f(sp_row), f(sp_col)]) + '\n')
        for fmt, (host, off) in pend.files:
            buf = host.numpy()
            for i, rec in enumerate(pend.recs):
                name = rec['name'] if fmt.startswith('pred') else os.path.splitext(rec['name'])[0] + '.jpg'
                with open(os.path.join(self.out, fmt % name), 'wb') as fh:
                    fh.write(buf[off[i]:off[i + 1]])
        if self.profile is not None:
            self.profile["encode_write"] = self.profile.get("encode_write", 0.0) + time.perf_counter() - t0
        return pend.recs

    def run(self, frames):
        torch = self._torch
        from .data.extract_flow import list_frames
        if isinstance(frames, (str, os.PathLike)):
            files = [(num, os.path.join(frames, name)) for num, name in list_frames(frames)]
        else:
            files = []
            for k, p in enumerate(frames):
                digits = ''.join(c for c in os.path.splitext(os.path.basename(p))[0] if c.isdigit())
                files.append((int(digits) if digits else k, os.fspath(p)))
        plans = chunk_plan(len(files), self.chunk)
        flags_file = load_fixsac(self.fixsac, len(files)) if self.fixsac not in ('all', 'auto') else None
        state = {'hw': None, 'gray': None, 'bgr': None, 'orig': None, 'flows': None, 'hidden': None,
                 'auto': OnlineFixation(self.fix_radius)}
        csv = None
        if self.out is not None:
            os.makedirs(self.out, exist_ok=True)
            csv = open(os.path.join(self.out, 'gaze.csv'), 'w')
            csv.write(CSV_HEADER + '\n')
        records, prev = [], None
        try:
            with torch.no_grad(), torch.cuda.device(self.device):
                for plan in plans:
                    cur = self._launch(plan, files, state, flags_file)
                    if prev is not None:
                        records += self._finish(prev, state, csv)
                    prev = cur
                if prev is not None:
                    records += self._finish(prev, state, csv)
                if self.lstm is not None:
                    from . import hipops as H
                    H.lstm_persist_check()       # a lost in-launch hand-off of the saccade-frame LSTM calls surfaces here
        finally:
            if csv is not None:
                csv.close()
        return records


def load_models(trained_model, trained_late, trained_lstm, device):
    """The three modules from their checkpoints, loaded as AT.__init__ / AT.reload_LSTM and LF.__init__ load them."""
    import torch
    from .models.late_fusion import late_fusion
    from .models.LSTMnet import lstmnet
    from .models.model_SP import model_SP
    from .utils import cfg, load_merged, make_layers
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20))
    load_merged(model, torch.load(trained_model, map_location='cpu', weights_only=False)['state_dict'], strict=False)
    late = late_fusion()
    load_merged(late, torch.load(trained_late, map_location='cpu', weights_only=False)['state_dict'])
    lstm = None
    if trained_lstm is not None:
        lstm = lstmnet()
        load_merged(lstm, torch.load(trained_lstm, map_location='cpu', weights_only=False))
        lstm.to(device)
    return model.to(device), lstm, late.to(device)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from .data.extract_flow import list_frames
    nframes = len(list_frames(args.framePath))
    try:
        predictable_frames(nframes)
    except ValueError as e:
        raise SystemExit(f"{args.framePath}: {e}")
    device = torch.device('cuda:' + args.device)
    lstm_file = args.trained_lstm if args.fixsac != 'all' else None          # 'all' never loads the LSTM
    model, lstm, late = load_models(args.trained_model, args.trained_late, lstm_file, device)
    pred = VideoPredictor(model, lstm, late, fixsac=args.fixsac, fix_radius=args.fix_radius, chunk=args.chunk,
                          crop_size=args.crop_size, flow_jpeg=args.flow_jpeg, handover_jpeg=args.handover_jpeg, bound=args.bound,
                          flow_params=args.params, overlay=args.overlay, save_maps=args.save_maps, out=args.out)
    try:
        records = pred.run(args.framePath)
    except ValueError as e:
        raise SystemExit(str(e))
    finally:
        pred.close()
    print(f"{len(records)} frames -> {os.path.join(args.out, 'gaze.csv')}")
    return records


if __name__ == '__main__':
    main()
