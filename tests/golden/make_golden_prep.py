#!/usr/bin/env python3
"""Generate tests/golden/dataset_prep.npz by running the REAL reference dataset-preparation scripts.

Runs only where the reference tree is available (REF below, read-only).  Nothing from the reference is copied: the fixture
holds the synthetic gaze logs written below (data) and what the reference scripts made of them.

    python tests/golden/make_golden_prep.py      # rewrites tests/golden/dataset_prep.npz byte-identically

  data/dataset_preprocessing.py (GTEA Gaze+)  runs as __main__ in a temporary directory holding gtea_gaze/, gtea_imgflow/
      and fixsac/: its live code writes fixsac/<video>.txt; its parsetxt is then called on every log.
  misc/gazedataset_gt.py (GTEA Gaze)          runs as __main__ in a temporary directory holding gazepositions/ and
      fixations/: it writes fixations/<name>_fixation.txt.
cv2 and skimage (image I/O, absent here) are stubbed; neither script calls them on its live path.

Keys (text as uint8 arrays):  gplus_<video>_log, gplus_<video>_fixsac, gplus_<video>_{gazex,gazey,nframe,fixsac}
                              gaze_<name>_track, gaze_<name>_fixation;  gplus_videos / gaze_names: '\\n'-joined names.
"""
import io
import os
import runpy
import sys
import tempfile
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

for name in ("cv2", "skimage", "skimage.io"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["skimage"].io = sys.modules["skimage.io"]


def line(x, y, frame, event, t=0):
    return f"{t}\tSMP\t1\t{x}\t{y}\t{frame}\t{event}\n"


def gplus_logs():
    """GTEA Gaze+ logs: columns 3 / 4 / 5 = x / y / frame, column 6 = event.  Every branch of parsetxt is visited."""
    logs = {}
    a = ["## exported gaze samples\n", "Time\tType\tTrial\tL POR X [px]\tL POR Y [px]\tFrame\tL Event Info\n",
         "# comment\n",
         line(1300.0, 400.0, 0, "Fixation"),             # out-of-range first sample -> frame 0 at (640, 480), label kept
         line(100.25, 200.75, 1, "Fixation"),
         line(102.25, 190.75, 1, "Fixation"),            # repeated frame, in range: averaged into the last entry
         line(-30.0, 190.0, 1, "Saccade"),               # repeated frame, out of range: ignored
         line(-0.5, 0.5, 2, "Saccade"),                  # round(-0.5) = 0 and round(0.5) = 0: in range, index -1 (wraps)
         line(1279.4, 959.4, 5, "Fixation"),             # gap: frames 3, 4 repeat frame 2's gaze and label
         line(1279.5, 500.0, 6, "Fixation"),             # round(1279.5) = 1280: out of range -> repeat, label 0
         line(600.0, 959.5, 7, "Fixation"),              # round(959.5) = 960: out of range
         line(600.0, 958.5, 8, "Fixation"),              # round(958.5) = 958: in range
         "T\trailer line\n",
         line(1278.5, 2.5, 9, "Blink"),
         line(0.49, 1.5, 9, "Blink"),                    # averaged
         line(640.5, 480.5, 10, "Fixation"),
         line(640.5, 481.5, 11, "Saccade"),
         line(641.0, 482.0, 11, "Fixation"),             # averaged; the label of the first sample stays
         line(10.0, 20.0, 14, "Saccade"),                # gap after a saccade: filled frames are labelled 0
         line(11.0, 21.0, 15, "Fixation")]
    logs["Alpha_Pasta"] = "".join(a)
    b = ["Time\tType\n", line(320.0, 240.0, 3, "Fixation")]       # the first frame need not be 0
    rs = np.random.RandomState(7)
    frame = 3
    for _ in range(60):
        frame += int(rs.choice([0, 1, 1, 1, 2, 4]))
        x = float(np.round(rs.uniform(-20, 1300), 2))
        y = float(np.round(rs.uniform(-20, 980), 2))
        b.append(line(x, y, frame, rs.choice(["Fixation", "Saccade", "Blink"])))
    logs["Beta_Pizza"] = "".join(b)
    return logs


def gaze_tracks():
    """GTEA Gaze tracks (x y per frame, 640 x 480): end zeros, interior zeros, out-of-frame values, x.5 coordinates,
    fixations of one sample (fix_num == 1 resets) and long fixations."""
    tracks = {}
    pts = [(0, 0), (100, 100), (110, 105), (300, 300), (305, 298), (500, 100), (0, 0), (0, 0), (520, 120),
           (0.5, 2.5), (700, 500), (639.5, 479.5), (640, 480), (200, 200), (0, 210), (205, 0), (210, 215),
           (400, 50), (600, 50), (0, 0)]
    tracks["Ahmad_Sandwich"] = "".join(f"{x} {y}\n" for x, y in pts)
    rs = np.random.RandomState(3)
    n = 80
    xs = np.cumsum(rs.normal(0, 25, n)) + 320
    ys = np.cumsum(rs.normal(0, 25, n)) + 240
    zero = rs.rand(n) < 0.15
    xs[zero] = 0
    ys[zero & (rs.rand(n) < 0.7)] = 0
    xs[0], ys[-1] = 0, 0
    tracks["Bea_Salad"] = "".join(f"{x:.2f} {y:.2f}\n" for x, y in zip(xs, ys))
    return tracks


def as_u8(text):
    return np.frombuffer(text.encode() if isinstance(text, str) else text, dtype=np.uint8)


def run_script(path, cwd):
    old = os.getcwd()
    os.chdir(cwd)
    try:
        return runpy.run_path(path, run_name="__main__")
    finally:
        os.chdir(old)


def save(name, **arrs):
    """np.savez_compressed layout with a fixed member timestamp, so that a rerun writes the same bytes."""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", name, "%.1f KB" % (os.path.getsize(path) / 1024))


def main():
    out = {}
    logs = gplus_logs()
    with tempfile.TemporaryDirectory() as tmp:
        for d in ("gtea_gaze", "gtea_imgflow", "fixsac"):
            os.makedirs(os.path.join(tmp, d))
        for video, text in logs.items():
            with open(os.path.join(tmp, "gtea_gaze", video + "_gaze.txt"), "w") as fh:
                fh.write(text)
            os.makedirs(os.path.join(tmp, "gtea_imgflow", video))
        g = run_script(os.path.join(REF, "data", "dataset_preprocessing.py"), tmp)
        for video, text in logs.items():
            out[f"gplus_{video}_log"] = as_u8(text)
            with open(os.path.join(tmp, "fixsac", video + ".txt"), "rb") as fh:
                out[f"gplus_{video}_fixsac"] = as_u8(fh.read())
            gx, gy, nf, fs = g["parsetxt"](os.path.join(tmp, "gtea_gaze", video + "_gaze.txt"))
            out[f"gplus_{video}_gazex"] = np.array(gx, np.float64)
            out[f"gplus_{video}_gazey"] = np.array(gy, np.float64)
            out[f"gplus_{video}_nframe"] = np.array(nf, np.int64)
            out[f"gplus_{video}_fixsac_list"] = np.array(fs, np.int64)
    out["gplus_videos"] = as_u8("\n".join(logs))

    tracks = gaze_tracks()
    with tempfile.TemporaryDirectory() as tmp:
        for d in ("gazepositions", "fixations"):
            os.makedirs(os.path.join(tmp, d))
        for name, text in tracks.items():
            with open(os.path.join(tmp, "gazepositions", name + ".txt"), "w") as fh:
                fh.write(text)
        run_script(os.path.join(REF, "misc", "gazedataset_gt.py"), tmp)
        for name, text in tracks.items():
            out[f"gaze_{name}_track"] = as_u8(text)
            with open(os.path.join(tmp, "fixations", name + "_fixation.txt"), "rb") as fh:
                out[f"gaze_{name}_fixation"] = as_u8(fh.read())
    out["gaze_names"] = as_u8("\n".join(tracks))
    save("dataset_prep.npz", **out)


if __name__ == "__main__":
    main()
