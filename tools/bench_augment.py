"""Augmentation in the resident gather (hipops.resident_gather_aug) measured against the plain gather of
the same run; lines are printed and written to --out (default profiles/augment_gather.txt):
  gather   B = 32, 224 x 224, all fields + NHWC-32 and abs-max, device events around --calls back-to-back calls (one region),
           the variants alternating region by region, median over --regions regions:
             plain      hipops.resident_gather, the yardstick (its kernel is not touched by the augmentation)
             identity   resident_gather_aug with explicit rows flip 0, dy = dx = 0, gain 1, bias 0 (bit-identical output)
             typical    the draw of flip=0.5,shift=16,contrast=0.2,brightness=0.1
             worst      explicit rows: flip everywhere, odd shifts up to 15 (two dwords per lane, reversed, border lanes)
  e2e      SP.trainSP steady-state step on a synthetic resident tree (tools/bench_resident.py's protocol: median interval
           between batches over --batches steps at B = 32), without and with --augment, alternating
Usage: python tools/bench_augment.py [--regions 9] [--calls 20] [--batches 24] [--out FILE] [--no-e2e]"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OUT = []
SPEC = "flip=0.5,shift=16,contrast=0.2,brightness=0.1"


def emit(line):
    OUT.append(line)
    print(line, flush=True)


def gather(regions, calls, B=32, H=224, W=224):
    import torch
    from egaze_amd import hipops as Hp
    dev = torch.device("cuda:0")
    frames = 256                                                   # 6 planes per frame, as the real pool
    g = torch.Generator().manual_seed(0)
    pool = torch.randint(0, 256, (frames * 6, H, W), dtype=torch.uint8, generator=g).to(dev)
    n = frames - 9
    t = torch.arange(9, frames)
    table = torch.empty((n, 22), dtype=torch.int64)
    table[:, 0] = 3 * t
    for m in range(10):
        table[:, 1 + 2 * m] = 3 * frames + 2 * (t - m)
        table[:, 2 + 2 * m] = 3 * frames + 2 * (t - m) + 1
    table[:, 21] = 5 * frames + t
    table = table.to(dev)
    idx = torch.randperm(n, generator=g)[:B].to(dev)
    spec = Hp.AugSpec.parse(SPEC, seed=1)
    one = np.array([1.0], dtype=np.float32).view(np.int32)[0]
    ident = torch.tensor([[0, 0, 0, one, 0]] * B, dtype=torch.int32, device=dev)
    worst = torch.tensor([[1, (-1) ** b * (2 * (b % 8) + 1), (-1) ** (b // 2) * (2 * (b % 8) + 1), one, 0] for b in range(B)],
                         dtype=torch.int32, device=dev)
    variants = {
        "plain": lambda: Hp.resident_gather(pool, table, idx, status_to={}),
        "identity": lambda: Hp.resident_gather_aug(pool, table, idx, spec, 0, params=ident, status_to={}),
        "typical": lambda: Hp.resident_gather_aug(pool, table, idx, spec, 0, status_to={}),
        "worst": lambda: Hp.resident_gather_aug(pool, table, idx, spec, 0, params=worst, status_to={}),
    }
    a, b = variants["plain"](), variants["identity"]()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[1]._egz_prepared[0], b[1]._egz_prepared[0])
    _, rows = Hp.resident_gather_aug(pool, table, idx, spec, 0, want_params=True)
    rows = rows.cpu()
    ts = {k: [] for k in variants}
    for r in range(regions + 2):                                   # two warm-up rounds
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ts[name].append(e0.elapsed_time(e1) / calls)
    nbytes = B * H * W * (24 + 24 * 4 + 32 * 4)
    emit(f"# gather: B = {B}, {H} x {W}, image + flow + gt + NHWC-32 + abs-max; ms per call (zero fill of the status and abs-max "
         f"words, kernel, status copy), {calls} calls per region, median of {regions} regions, variants alternating; "
         f"counted traffic {nbytes / 1e6:.0f} MB per call")
    emit(f"# typical draw of this batch: {int(rows[:, 0].sum())} of {B} flipped, |dy| <= {int(rows[:, 1].abs().max())}, "
         f"|dx| <= {int(rows[:, 2].abs().max())}, {int((rows[:, 2] % 4 != 0).sum())} samples with dx % 4 != 0")
    base = float(np.median(ts["plain"]))
    for name in variants:
        ms = float(np.median(ts[name]))
        emit(f"gather {name:9s} median {ms:.4f} ms  (min {min(ts[name]):.4f}, max {max(ts[name]):.4f})  "
             f"{nbytes / ms / 1e6:6.0f} GB/s  x{ms / base:.3f} of plain"
             + (f"  bit-identical with plain: {bool(same)}" if name == "identity" else ""))
    return {k: float(np.median(v)) for k, v in ts.items()}


class _Timed:
    """tools/bench_jpeg._Timed with the loader's dataset in view (SP.trainSP looks for it to enter dataset.augmenting)."""

    def __init__(self, inner):
        self.inner, self.stamps = inner, inner.stamps

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        return iter(self.inner)

    @property
    def dataset(self):
        return self.inner.loader.dataset

    @property
    def loader(self):
        return self.inner.loader


def e2e(batches, B=32):
    import torch
    import bench_jpeg as J
    from egaze_amd import hipops as Hp
    from egaze_amd.SP import SP
    from egaze_amd.data.resident import ResidentSTDataset
    streams = J.make_streams()
    spec = Hp.AugSpec.parse(SPEC, seed=1)
    res = {"plain": [], "augment": []}
    with tempfile.TemporaryDirectory() as root:
        J.fake_vgg(os.path.join(root, "vgg.pth"))
        os.environ["EGAZE_VGG16_BN"] = os.path.join(root, "vgg.pth")
        args = J.write_tree(os.path.join(root, "tree"), streams, B * batches)
        ds = ResidentSTDataset(*args, raw_u8=True, decode="gpu").fill("cuda:0")
        for mode in ("plain", "augment", "plain", "augment"):
            torch.manual_seed(0)
            sp = SP(lr=1e-4, save_path=os.path.join(root, "save"), batch_size=B, device="0", resume="0", traindata=ds,
                    valdata=ds, augment=spec if mode == "augment" else None)
            sp.trainSP()                                           # warm: allocations, packings
            timed = _Timed(J._Timed(sp.STTrainLoader))
            sp.STTrainLoader = timed
            sp.trainSP()
            torch.cuda.synchronize()
            d = np.diff(timed.stamps)[2:]
            res[mode].append(float(np.median(d)) * 1e3)
            emit(f"e2e trainSP B={B} {mode:8s} median {np.median(d) * 1e3:.2f} ms / step  (min {d.min() * 1e3:.2f}, "
                 f"max {d.max() * 1e3:.2f}) over {len(d)} steps  {B / float(np.median(d)):.0f} frames/s")
            del sp
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--regions", type=int, default=9)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--batches", type=int, default=24)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_gather.txt"))
    p.add_argument("--no-e2e", action="store_true")
    a = p.parse_args()
    if a.regions < 5:
        raise SystemExit("bench_augment: at least 5 regions per variant")
    import torch
    import egaze_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs the GPU (no timing is taken on a CPU)")
    props = torch.cuda.get_device_properties(0)
    emit(f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, "
         f"{props.total_memory / 2 ** 30:.0f} GiB), torch {torch.__version__}, HIP {torch.version.hip}")
    emit(f"# augmentation spec of 'typical' and of the training loop: {SPEC}, seed 1")
    g = gather(a.regions, a.calls)
    emit(f"# ratio typical / plain: {g['typical'] / g['plain']:.3f}; identity / plain: {g['identity'] / g['plain']:.3f}; "
         f"worst / plain: {g['worst'] / g['plain']:.3f}")
    if not a.no_e2e:
        emit("# e2e: SP.trainSP, every layer trained, median interval between batches, same resident pool, modes alternating")
        r = e2e(a.batches)
        emit(f"# ratio augment / plain per step: {np.mean(r['augment']) / np.mean(r['plain']):.4f} "
             f"(plain {r['plain']}, augment {r['augment']})")
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
