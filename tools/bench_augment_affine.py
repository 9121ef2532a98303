"""Scale and rotation jitter in the resident gather (egz_resident_gather_affine through hipops.resident_gather_aug, DESIGN.md
section 21) measured against the plain and the section-20 gathers of the same run; lines are printed and written to --out
(default profiles/augment_affine.txt).  The protocol is tools/bench_augment.py's:
  gather   B = 32, 224 x 224, all fields + NHWC-32 and abs-max, device events around --calls back-to-back calls (one region),
           the variants alternating region by region, median over --regions regions:
             plain            hipops.resident_gather, the yardstick
             aug_identity     egz_resident_gather_aug, explicit rows flip 0, dy = dx = 0, gain 1, bias 0
             aug_typical      egz_resident_gather_aug, the draw of flip=0.5,shift=16,contrast=0.2,brightness=0.1
             affine_identity  egz_resident_gather_affine, the identity as (B, 7) rows (g = 1, theta = 0): the integer-offset path
             affine_typical   egz_resident_gather_affine, the draw of the spec above with scale=0.15,rotate=10
             affine_worst     egz_resident_gather_affine, every sample at g = 0.5, theta = pi / 4 (strides of 2 source pixels)
  e2e      SP.trainSP steady-state step on a synthetic resident tree, with the section-20 spec and with the two new keys added,
           alternating
Usage: python tools/bench_augment_affine.py [--regions 9] [--calls 20] [--batches 24] [--out FILE] [--no-e2e]"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_augment as BA  # noqa: E402

emit = BA.emit
SPEC = BA.SPEC
AFFINE = SPEC + ",scale=0.15,rotate=10"


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
    spec, affine = Hp.AugSpec.parse(SPEC, seed=1), Hp.AugSpec.parse(AFFINE, seed=1)
    bits = lambda v: int(np.array([v], dtype=np.float32).view(np.int32)[0])
    ident5 = torch.tensor([[0, 0, 0, bits(1), 0]] * B, dtype=torch.int32, device=dev)
    ident7 = torch.tensor([[0, 0, 0, bits(1), 0, bits(1), 0]] * B, dtype=torch.int32, device=dev)
    worst = torch.tensor([[0, 0, 0, bits(1), 0, bits(0.5), bits(np.pi / 4)]] * B, dtype=torch.int32, device=dev)
    variants = {
        "plain": lambda: Hp.resident_gather(pool, table, idx, status_to={}),
        "aug_identity": lambda: Hp.resident_gather_aug(pool, table, idx, spec, 0, params=ident5, status_to={}),
        "aug_typical": lambda: Hp.resident_gather_aug(pool, table, idx, spec, 0, status_to={}),
        "affine_identity": lambda: Hp.resident_gather_aug(pool, table, idx, affine, 0, params=ident7, status_to={}),
        "affine_typical": lambda: Hp.resident_gather_aug(pool, table, idx, affine, 0, status_to={}),
        "affine_worst": lambda: Hp.resident_gather_aug(pool, table, idx, affine, 0, params=worst, status_to={}),
    }
    a, b = variants["aug_identity"](), variants["affine_identity"]()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[1]._egz_prepared[0], b[1]._egz_prepared[0])
    _, rows = Hp.resident_gather_aug(pool, table, idx, affine, 0, want_params=True)
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
         f"counted traffic {nbytes / 1e6:.0f} MB per call (the pool bytes counted once)")
    gs, th = rows[:, 5].contiguous().view(torch.float32), rows[:, 6].contiguous().view(torch.float32)
    emit(f"# typical draw of this batch: {int(rows[:, 0].sum())} of {B} flipped, |dy| <= {int(rows[:, 1].abs().max())}, "
         f"|dx| <= {int(rows[:, 2].abs().max())}, g in {float(gs.min()):.3f} .. {float(gs.max()):.3f}, theta in "
         f"{float(th.min()) * 180 / np.pi:.2f} .. {float(th.max()) * 180 / np.pi:.2f} degrees")
    base = float(np.median(ts["plain"]))
    for name in variants:
        ms = float(np.median(ts[name]))
        emit(f"gather {name:15s} median {ms:.4f} ms  (min {min(ts[name]):.4f}, max {max(ts[name]):.4f})  "
             f"{nbytes / ms / 1e6:6.0f} GB/s  x{ms / base:.3f} of plain"
             + (f"  bit-identical with aug_identity: {bool(same)}" if name == "affine_identity" else ""))
    for name in variants:
        emit(f"# regions {name:15s} " + " ".join(f"{v:.4f}" for v in ts[name]))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}


def e2e(batches, B=32):
    import torch
    import bench_jpeg as J
    from egaze_amd import hipops as Hp
    from egaze_amd.SP import SP
    from egaze_amd.data.resident import ResidentSTDataset
    streams = J.make_streams()
    specs = {"augment": Hp.AugSpec.parse(SPEC, seed=1), "affine": Hp.AugSpec.parse(AFFINE, seed=1)}
    res = {k: [] for k in specs}
    with tempfile.TemporaryDirectory() as root:
        J.fake_vgg(os.path.join(root, "vgg.pth"))
        os.environ["EGAZE_VGG16_BN"] = os.path.join(root, "vgg.pth")
        args = J.write_tree(os.path.join(root, "tree"), streams, B * batches)
        ds = ResidentSTDataset(*args, raw_u8=True, decode="gpu").fill("cuda:0")
        for mode in ("augment", "affine", "augment", "affine"):
            torch.manual_seed(0)
            sp = SP(lr=1e-4, save_path=os.path.join(root, "save"), batch_size=B, device="0", resume="0", traindata=ds,
                    valdata=ds, augment=specs[mode])
            sp.trainSP()                                           # warm: allocations, packings
            timed = BA._Timed(J._Timed(sp.STTrainLoader))
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_affine.txt"))
    p.add_argument("--no-e2e", action="store_true")
    a = p.parse_args()
    if a.regions < 5:
        raise SystemExit("bench_augment_affine: at least 5 regions per variant")
    import torch
    import egaze_amd  # noqa: F401
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment_affine: needs the GPU (no timing is taken on a CPU)")
    props = torch.cuda.get_device_properties(0)
    emit(f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, "
         f"{props.total_memory / 2 ** 30:.0f} GiB), torch {torch.__version__}, HIP {torch.version.hip}")
    emit(f"# specs: section 20 '{SPEC}', with the new keys '{AFFINE}', seed 1")
    g = gather(a.regions, a.calls)
    ai, fi = g["aug_identity"], g["affine_identity"]
    emit(f"# identity rows: affine kernel {fi[0]:.4f} ms against section-20 kernel {ai[0]:.4f} ms (its regions {ai[1]:.4f} .. "
         f"{ai[2]:.4f}): {'inside' if fi[0] <= ai[2] else 'ABOVE'} its spread; typical affine / typical section 20: "
         f"{g['affine_typical'][0] / g['aug_typical'][0]:.3f}; worst / plain: {g['affine_worst'][0] / g['plain'][0]:.3f}")
    if not a.no_e2e:
        emit("# e2e: SP.trainSP, every layer trained, median interval between batches, same resident pool, modes alternating")
        r = e2e(a.batches)
        emit(f"# ratio affine / augment per step: {np.mean(r['affine']) / np.mean(r['augment']):.4f} "
             f"(augment {r['augment']}, affine {r['affine']})")
    with open(a.out, "w") as f:
        f.write("\n".join(BA.OUT) + "\n")


if __name__ == "__main__":
    main()
