"""egz_gaze_gt_maps (csrc/gaze_gt.hip) on the GPU: the ground-truth gaze maps of the reference's dataset preparation.
Full-resolution maps bit-identical to scipy.ndimage.gaussian_filter plus the reference's normalisation; resized maps
bit-identical to the INTER_AREA restatement of test_dataset_prep_host.py in both modes; batch independence; argument checks;
and the dataset_preprocessing CLI end to end on a synthetic GTEA Gaze+ tree, read back by STDataset and trained on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dataset_prep_host as R  # noqa: E402  (the numpy restatement of the render)

DEV = "cuda:0"
GEOMS = {"gplus": R.GPLUS, "gaze": R.GAZE}


def _maps(pos, geom, **kw):
    from egaze_amd import hipops
    hw, sigma, mode = geom
    rows = torch.tensor([p[0] for p in pos], dtype=torch.int32, device=DEV)
    cols = torch.tensor([p[1] for p in pos], dtype=torch.int32, device=DEV)
    return hipops.gaze_gt_maps(rows, cols, hw, sigma, (224, 224), mode, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gplus", "gaze"])
def test_fullres_bit_identical_to_scipy(name):
    from scipy import ndimage
    hw, sigma, mode = GEOMS[name]
    pos = R.positions(hw, sigma)
    assert len(pos) >= 12
    _, _, full = _maps(pos, GEOMS[name], want_fullres=True)
    full = full.cpu().numpy()
    for n, (r, c) in enumerate(pos):
        imp = np.zeros(hw); imp[r, c] = 1
        ref = ndimage.gaussian_filter(imp, sigma)
        ref -= np.min(ref); ref /= np.max(ref); ref *= 255
        assert np.array_equal(full[n], ref), (name, r, c, np.abs(full[n] - ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gplus", "gaze"])
def test_resized_maps_bit_identical_to_restatement(name):
    hw, sigma, mode = GEOMS[name]
    pos = R.positions(hw, sigma)
    u8, f64, _ = _maps(pos, GEOMS[name], want_f64=True)
    u8, f64 = u8.cpu().numpy(), f64.cpu().numpy()
    for n, (r, c) in enumerate(pos):
        ref_f, ref_u8 = R.render(r, c, hw, sigma, mode)
        assert np.array_equal(f64[n], ref_f), (name, r, c, np.abs(f64[n] - ref_f).max())
        assert np.array_equal(u8[n], ref_u8), (name, r, c)
        assert u8[n].max() >= 250 and u8[n].min() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gplus", "gaze"])
def test_batch_of_1000_equals_single_frames(name):
    hw, sigma, _ = GEOMS[name]
    rs = np.random.RandomState(11)
    pos = list(zip(rs.randint(0, hw[0], 1000).tolist(), rs.randint(0, hw[1], 1000).tolist()))
    pos[0], pos[999] = (0, 0), (hw[0] - 1, hw[1] - 1)
    batch, bf, _ = _maps(pos, GEOMS[name], want_f64=True)
    for n in (0, 1, 500, 999):
        one, of, _ = _maps([pos[n]], GEOMS[name], want_f64=True)
        assert torch.equal(batch[n], one[0]) and torch.equal(bf[n], of[0])
    u8, _, _ = _maps(pos, GEOMS[name])
    assert torch.equal(u8, batch)          # with and without the optional outputs


@pytest.mark.gpu
def test_invalid_arguments_raise():
    from egaze_amd import hipops
    from egaze_amd._lib import EgazeHipError, LIB
    r = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        hipops.gaze_gt_maps(r.cpu(), r.cpu(), (960, 1280), 70.0)
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r.float(), r, (960, 1280), 70.0)
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, r[:1], (960, 1280), 70.0)
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, torch.tensor([1, 1280], dtype=torch.int32, device=DEV), (960, 1280), 70.0)
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, -r, (960, 1280), 70.0)
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, r, (960, 1280), 70.0, mode=2)
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, r, (200, 1280), 70.0)              # radius 280 >= 200
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, r, (960, 1280), 70.0, out_hw=(1000, 224))
    with pytest.raises(ValueError):
        hipops.gaze_gt_maps(r, r, (960, 1280), 0.0)
    # the C entry checks on its own
    gw, rad = hipops._gauss_weights(DEV, 70.0)
    (yo, ys, ya), (xo, xs, xa) = hipops._area_tables(DEV, (960, 1280), (224, 224))
    pos = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.empty((2, 224, 224), dtype=torch.uint8, device=DEV)
    args = [pos.data_ptr(), 2, 960, 1280, gw.data_ptr(), rad, xo.data_ptr(), xs.data_ptr(), xa.data_ptr(), xs.numel(),
            yo.data_ptr(), ys.data_ptr(), ya.data_ptr(), ys.numel(), 0, 224, 224, out.data_ptr(), None, None, None]
    bad = {14: 3, 5: 960, 1: 0, 17: None, 2: 9000}
    for i, v in bad.items():
        a = list(args); a[i] = v
        with pytest.raises(EgazeHipError):
            hipops.check(LIB.egz_gaze_gt_maps(*a), "egz_gaze_gt_maps")
    hipops.check(LIB.egz_gaze_gt_maps(*args), "egz_gaze_gt_maps")
    torch.cuda.synchronize()


def _synthetic_tree(tmp_path, gold):
    """gtea_gaze/ from the golden logs and gtea_imgflow/<video>/ with one img / flow_x / flow_y frame per logged frame + 1."""
    from PIL import Image
    rs = np.random.RandomState(0)
    videos = R._text(gold["gplus_videos"]).split("\n")
    (tmp_path / "gtea_gaze").mkdir()
    for video in videos:
        (tmp_path / "gtea_gaze" / (video + "_gaze.txt")).write_bytes(gold[f"gplus_{video}_log"].tobytes())
        d = tmp_path / "gtea_imgflow" / video
        d.mkdir(parents=True)
        for n in range(1, len(gold[f"gplus_{video}_nframe"]) + 2):
            Image.fromarray(rs.randint(0, 256, (224, 224, 3)).astype(np.uint8)).save(str(d / f"img_{n:05d}.jpg"))
            for ax in "xy":
                Image.fromarray(rs.randint(0, 256, (224, 224)).astype(np.uint8)).save(str(d / f"flow_{ax}_{n:05d}.jpg"))
    return videos


@pytest.mark.gpu
def test_cli_end_to_end_feeds_stdataset_and_sp_step(tmp_path):
    from PIL import Image
    from torch.utils.data import DataLoader
    from egaze_amd.data import dataset_preprocessing as D
    from egaze_amd.data.STdatas import STDataset, stage_batch
    from egaze_amd.models.model_SP import model_SP
    from egaze_amd.utils import make_layers, cfg
    from egaze_amd.floss import floss
    from egaze_amd.optim import FusedAdam
    gold = R._golden()
    videos = _synthetic_tree(tmp_path, gold)
    p = {k: str(tmp_path / v) for k, v in (("gaze", "gtea_gaze"), ("flow", "gtea_imgflow"), ("img", "gtea_images"),
                                           ("gt", "gtea_gts"), ("fs", "fixsac"))}
    D.main(["--gazePath", p["gaze"], "--flowPath", p["flow"], "--imagePath", p["img"], "--gtPath", p["gt"],
            "--fixsacPath", p["fs"], "--gt-format", "png", "--workers", "4"])
    for video in videos:
        assert open(os.path.join(p["fs"], video + ".txt"), "rb").read() == gold[f"gplus_{video}_fixsac"].tobytes()
        gx, gy = gold[f"gplus_{video}_gazex"].tolist(), gold[f"gplus_{video}_gazey"].tolist()
        maps = D.render_maps(gx[1:], gy[1:])
        for i in range(1, len(gx)):
            img = f"img_{i + 1:05d}"
            gt = np.asarray(Image.open(os.path.join(p["gt"], f"{video}_gt_{img}.png")))
            assert np.array_equal(gt, maps[i - 1]), (video, i)
            assert open(os.path.join(p["img"], f"{video}_{img}.jpg"), "rb").read() == \
                open(os.path.join(p["flow"], video, img + ".jpg"), "rb").read()
        # the maps are the reference's: spot-check two frames against the restatement
        for i in (1, len(gx) - 1):
            r, c = D.impulse_index(gy[i], 960), D.impulse_index(gx[i], 1280)
            assert np.array_equal(maps[i - 1], R.render(r, c, (960, 1280), 70.0, 0)[1])
    assert len(os.listdir(p["gt"])) == sum(len(gold[f"gplus_{v}_nframe"]) - 1 for v in videos)

    # the tree feeds STDataset as gaze_full lays it out; listed gts have their 10 flow frames (number >= 10)
    gts = sorted(g for g in os.listdir(p["gt"]) if int(g[-9:-4]) >= 10)
    ims = [g.replace("_gt_", "_").replace(".png", ".jpg") for g in gts]
    assert all(os.path.exists(os.path.join(p["img"], m)) for m in ims)
    args = (p["flow"], p["img"], p["gt"], sorted(os.listdir(p["flow"])), ims, gts, sorted(os.listdir(p["fs"])), p["fs"])
    ds = STDataset(*args)
    for n in (0, len(gts) - 1):
        s = ds[n]
        ref = np.asarray(Image.open(os.path.join(p["gt"], gts[n])))
        assert torch.equal(s["gt"], torch.from_numpy(ref).float().div(255).unsqueeze(0))
        assert tuple(s["flow"].shape) == (20, 224, 224) and tuple(s["image"].shape) == (3, 224, 224)

    torch.manual_seed(0)
    model = model_SP(make_layers(cfg['D'], 3), make_layers(cfg['D'], 20)).to(DEV).train()
    opt = FusedAdam(model.parameters(), lr=1e-7)
    sample = next(iter(DataLoader(STDataset(*args, raw_u8=True), batch_size=2, shuffle=False)))
    x_s, x_t, target = stage_batch(sample, torch.device(DEV))
    out = model(x_s, x_t)
    loss = floss()(out, target.view(out.size()))
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
