"""Depth supervision from tie points on the GPU (datasets/satellite_depth.py:51-129): load_depth_supervision
on the committed scene against the arrays the reference's SatelliteDataset_depth built from it (tests/golden/depth_supervision/),
each kernel against the numpy restatement (tests/depth_supervision_reference.py), determinism, and the error paths."""
import math
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import rpc_oracle as R
from tests import depth_supervision_reference as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_supervision")


def _fixture():
    z = np.load(os.path.join(SCENE, "reference.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def _scene_copy(tmp_path, name="scene"):
    root = str(tmp_path / name)
    shutil.copytree(SCENE, root)
    os.remove(os.path.join(root, "reference.npz"))
    return root


def test_load_depth_supervision_matches_the_reference():
    from satnerf_amd import data

    g = _fixture()
    rays, depths, ts, e, w = (t.cpu().numpy() for t in data.load_depth_supervision(SCENE, device=DEV, return_point_weights=True))
    rng = float(g["range"])
    assert rays.shape == g["all_rays"].shape and depths.shape == g["all_depths"].shape and ts.dtype == np.int64
    assert np.array_equal(ts, g["all_ids"][:, 0].astype(np.int64))
    # the test_rpc.py gates: the origin carries one fp32 ulp of ECEF (0.5 m) over the range, everything else fp32 rounding
    assert np.abs(rays[:, 0:3] - g["all_rays"][:, 0:3]).max() <= 0.5 / rng + 1e-6
    assert np.abs(rays[:, 3:6] - g["all_rays"][:, 3:6]).max() < 2e-6
    assert np.abs(rays[:, 6:8] - g["all_rays"][:, 6:8]).max() < 2e-6
    assert np.abs(rays[:, 8:11] - g["all_rays"][:, 8:11]).max() < 1e-6
    assert np.abs(depths[:, 0] - g["all_depths"][:, 0]).max() <= np.sqrt(3) * 0.5 / rng + 1e-6
    assert np.abs(e - g["e"]).max() <= 2e-6 * np.abs(g["e"]).max()
    assert np.abs(w - g["kp_weights"]).max() <= 5e-6 and np.abs(depths[:, 1] - g["all_depths"][:, 1]).max() <= 5e-6


def test_rays_at_integer_coordinates_are_the_image_rays_bit_for_bit():
    from satnerf_amd import ops

    h, w = 48, 64
    rpc = R.synthetic_rpc(0, height=h, width=w)
    center, rng = [796912.4, -5453871.2, 3200310.9], 310.0
    full, _ = ops.rpc_rays(rpc, w, h, -25.0, 60.0, center, rng, 52.0, 141.0, DEV)
    pick = torch.randperm(h * w, generator=torch.Generator().manual_seed(1))[:1000]
    colrow = torch.stack([pick % w, pick // w], 1).double().to(DEV)
    got = ops.rpc_rays_at(rpc, colrow, -25.0, 60.0, center, rng, 52.0, 141.0)
    assert torch.equal(got.cpu().view(torch.int32), full.cpu()[pick].view(torch.int32))


def _random_case(n_cams=16, n_pts=50_000, per_cam=25_000, seed=7):
    g = np.random.default_rng(seed)
    lat = 30.30 + g.uniform(-0.5, 0.5, n_pts) * 0.0035
    lon = -81.66 + g.uniform(-0.5, 0.5, n_pts) * 0.0040
    alt = g.uniform(-15.0, 45.0, n_pts)
    pts3d = np.stack(R.latlon_to_ecef(lat, lon, alt), 1)
    cams = []
    for t in range(n_cams):
        rpc = R.synthetic_rpc(200 + t, height=400, width=400)
        idx = g.integers(0, n_pts, per_cam)  # with repeats: duplicates within one camera
        col, row = R.projection(rpc, lon[idx], lat[idx], alt[idx])
        colrow = np.stack([col, row], 1) + g.normal(0.0, 0.5, (per_cam, 2))
        cams.append((rpc, colrow, idx))
    return pts3d, cams


def test_reprojection_errors_within_one_ulp_and_weights_repeatable():
    from satnerf_amd import ops

    pts3d, cams = _random_case()
    p_dev = torch.from_numpy(pts3d).to(DEV)
    errs, idxs, tss = [], [], []
    for t, (rpc, colrow, idx) in enumerate(cams):
        cr, ix = torch.from_numpy(colrow).to(DEV), torch.from_numpy(idx).to(DEV)
        got = ops.reprojection_errors(rpc, cr, ix, p_dev).cpu().numpy()
        want = D.reprojection_errors(rpc, colrow, pts3d[idx]).astype(np.float32)
        # one fp32 ulp; for errors near 0 the floor is fp64's resolution of the projected coordinate (one ulp of a latitude
        # near 30 degrees is ~2e-10 px after the RPC normalisation), where host and device libm may differ
        d = np.abs(got - want)
        assert (d <= np.maximum(np.spacing(want), 1e-8)).all(), (d.max(), want[np.argmax(d - np.spacing(want))])
        errs.append(got), idxs.append(idx), tss.append(np.full(idx.size, t, np.int64))
    assert sum(e.size for e in errs) >= 400_000
    err, idx, ts = (torch.from_numpy(np.concatenate(a)).to(DEV) for a in (errs, idxs, tss))
    runs = [ops.keypoint_weights(idx, ts, err, pts3d.shape[0], len(cams)) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # against the restatement on the same fp32 errors: last observation per (point, camera), fp64 sums rounded once
    errmat = np.zeros((pts3d.shape[0], len(cams)), np.float32)
    for t, (e, ix) in enumerate(zip(errs, idxs)):
        errmat[ix, t] = e
    e64 = np.zeros(pts3d.shape[0])
    for t in range(len(cams)):
        e64 += errmat[:, t]
    e_want = e64.astype(np.float32)
    e_mean = np.float32(e_want.astype(np.float64).sum() / pts3d.shape[0])
    e_got, w_got, em_got = (t.cpu().numpy() for t in runs[0])
    assert np.array_equal(e_got, e_want) and em_got[0] == e_mean
    assert np.abs(w_got - np.exp(-(e_want / e_mean) ** 2)).max() <= 1e-6


def test_keypoint_weights_with_more_partials_than_threads():
    """n_pts = 65 537 gives 257 per-workgroup partials, so finalize's strided sum takes a second trip (the 50 000-point case has 196).
    The same restatement and bounds as above, on random fp32 errors of 3 cameras, and two runs bit-equal."""
    from satnerf_amd import ops

    n_pts, n_cams, per_cam = 65_537, 3, 60_000
    g = np.random.default_rng(11)
    errs = [g.uniform(0.0, 2.0, per_cam).astype(np.float32) for _ in range(n_cams)]
    idxs = [g.integers(0, n_pts, per_cam) for _ in range(n_cams)]  # with repeats
    idxs[0][-1] = n_pts - 1  # the lone point of the last workgroup is observed
    tss = [np.full(per_cam, t, np.int64) for t in range(n_cams)]
    err, idx, ts = (torch.from_numpy(np.concatenate(a)).to(DEV) for a in (errs, idxs, tss))
    runs = [ops.keypoint_weights(idx, ts, err, n_pts, n_cams) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    errmat = np.zeros((n_pts, n_cams), np.float32)
    for t, (e, ix) in enumerate(zip(errs, idxs)):
        errmat[ix, t] = e
    e64 = np.zeros(n_pts)
    for t in range(n_cams):
        e64 += errmat[:, t]
    e_want = e64.astype(np.float32)
    e_mean = np.float32(e_want.astype(np.float64).sum() / n_pts)
    e_got, w_got, em_got = (t.cpu().numpy() for t in runs[0])
    print("e mismatches", int((e_got != e_want).sum()), "e_mean", em_got[0], e_mean, "max |dw|", np.abs(w_got - np.exp(-(e_want / e_mean) ** 2)).max())
    assert np.array_equal(e_got, e_want) and em_got[0] == e_mean
    assert np.abs(w_got - np.exp(-(e_want / e_mean) ** 2)).max() <= 1e-6


def test_duplicate_observation_keeps_the_last():
    from satnerf_amd import ops

    idx = torch.tensor([3, 1, 3, 3, 0], dtype=torch.int64, device=DEV)
    cam = torch.tensor([0, 0, 0, 1, 1], dtype=torch.int64, device=DEV)
    err = torch.tensor([1.0, 2.0, 0.5, 4.0, 8.0], device=DEV)
    e, w, em = ops.keypoint_weights(idx, cam, err, 5, 2)
    assert e.cpu().tolist() == [8.0, 2.0, 0.0, 4.5, 0.0] and em.item() == pytest.approx(14.5 / 5)


def _chord_scene(n_img=3, k=300, seed=3):
    """A scene with noise-free keypoints: each tie point lies on the fp64 chord (max_alt -> min_alt) its keypoint's ray is built from."""
    g = np.random.default_rng(seed)
    images, pts = [], []
    lo_alt, hi_alt = -20.0, 60.0
    for t in range(n_img):
        rpc = R.synthetic_rpc(40 + t, height=300, width=300)
        col, row = g.uniform(20, 280, k), g.uniform(20, 280, k)
        lon, lat = R.localization(rpc, col, row, np.full(k, hi_alt))
        near = np.stack(R.latlon_to_ecef(lat, lon, np.full(k, hi_alt)), 1)
        lon, lat = R.localization(rpc, col, row, np.full(k, lo_alt))
        far = np.stack(R.latlon_to_ecef(lat, lon, np.full(k, lo_alt)), 1)
        pts.append(near + g.uniform(0.0, 1.0, (k, 1)) * (far - near))
        images.append({"rpc": {a: (v.tolist() if isinstance(v, np.ndarray) else v) for a, v in rpc.items()}, "min_alt": lo_alt,
                       "max_alt": hi_alt, "sun_elevation": 50.0, "sun_azimuth": 150.0,
                       "keypoints": {"2d_coordinates": np.stack([col, row], 1).tolist(), "pts3d_indices": list(range(t * k, (t + 1) * k))}})
    pts3d = np.concatenate(pts)
    return images, pts3d, torch.tensor(pts3d.mean(0).tolist()), 300.0  # centre rounded to fp32 as read_scene_loc does


def test_tie_points_lie_on_their_rays():
    from satnerf_amd import data

    images, pts3d, center, rng = _chord_scene()
    rays, depths, ts = (t.cpu().numpy().astype(np.float64) for t in data.depth_supervision_from_keypoints(images, pts3d, center, rng, DEV))
    p = (pts3d - center.double().numpy()) / rng  # pts3d rows are in observation order
    hit = rays[:, 0:3] + rays[:, 3:6] * depths[:, :1]
    quant = np.sqrt(3) * 0.5 / rng + 1e-6  # fp32 ECEF (0.5 m ulp) of the origin and of the tie point, over the range
    assert np.linalg.norm(hit - p, axis=1).max() <= quant
    assert (depths[:, 0] <= rays[:, 7] + quant).all()  # between near (0) and far


def test_two_runs_are_bitwise_equal_and_blank_lines_are_skipped(tmp_path):
    from satnerf_amd import data

    a = data.load_depth_supervision(SCENE, device=DEV, return_point_weights=True)
    root = _scene_copy(tmp_path)
    with open(os.path.join(root, "train.txt")) as f:
        names = f.read().split("\n")
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(names[:3] + [""] + names[3:]) + "\n")
    b = data.load_depth_supervision(root, device=DEV, return_point_weights=True)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.cpu().view(torch.uint8), y.cpu().view(torch.uint8))


def test_an_image_without_keypoints_counts_as_a_camera():
    from satnerf_amd import data

    images, pts3d, center, rng = D.load_scene(SCENE)
    images[1] = dict(images[1], keypoints={"2d_coordinates": [], "pts3d_indices": []})
    rays, depths, ts = data.depth_supervision_from_keypoints(images, pts3d, torch.from_numpy(center), float(rng), DEV)
    ts = ts.cpu().numpy()
    assert 1 not in set(ts.tolist()) and ts.max() == len(images) - 1
    assert rays.shape[0] == depths.shape[0] == sum(len(d["keypoints"]["pts3d_indices"]) for d in images)


def test_error_paths(tmp_path):
    from satnerf_amd import data

    root = _scene_copy(tmp_path, "nopts")
    os.remove(os.path.join(root, "pts3d.npy"))
    with pytest.raises(FileNotFoundError, match="Could not find .*pts3d.npy"):
        data.load_depth_supervision(root, device=DEV)
    root = _scene_copy(tmp_path, "noloc")
    os.remove(os.path.join(root, "scene.loc"))
    with pytest.raises(FileNotFoundError, match="scene.loc.*required"):
        data.load_depth_supervision(root, device=DEV)
    images, pts3d, center, rng = D.load_scene(SCENE)
    center = torch.from_numpy(center)
    bad = [dict(d) for d in images]
    del bad[4]["keypoints"]
    with pytest.raises(ValueError, match="No 'keypoints' field was found in img_04.json"):
        data.depth_supervision_from_keypoints(bad, pts3d, center, rng, DEV, names=[f"img_{k:02d}.json" for k in range(len(bad))])
    for wrong in (pts3d.shape[0], -1):
        bad = [dict(d) for d in images]
        bad[2]["keypoints"] = dict(bad[2]["keypoints"], pts3d_indices=bad[2]["keypoints"]["pts3d_indices"][:-1] + [wrong])
        with pytest.raises(ValueError, match="pts3d_indices must lie in"):
            data.depth_supervision_from_keypoints(bad, pts3d, center, rng, DEV)
    empty = [dict(d, keypoints={"2d_coordinates": [], "pts3d_indices": []}) for d in images]
    with pytest.raises(ValueError, match="mean reprojection error"):
        data.depth_supervision_from_keypoints(empty, pts3d, center, rng, DEV)
    bad = [dict(d) for d in images]
    cr = [list(c) for c in bad[0]["keypoints"]["2d_coordinates"]]
    cr[0][0] = float("nan")
    bad[0]["keypoints"] = dict(bad[0]["keypoints"], **{"2d_coordinates": cr})
    with pytest.raises(ValueError, match="mean reprojection error"):
        data.depth_supervision_from_keypoints(bad, pts3d, center, rng, DEV)


def test_trainer_step_with_the_loaded_depth_bank():
    from oracle import satnerf_oracle as O
    from satnerf_amd import data
    from satnerf_amd.models import load_model
    from satnerf_amd.train import Trainer

    rays_d, depths, ts_d = data.load_depth_supervision(SCENE, device=DEV)
    args = O.default_args(mlp_mode="bf16x3", ds_lambda=1000.0)
    m = load_model(args)
    m.load_state_dict(O.procedural_satnerf_params(256, 4, seed=31))
    emb = torch.nn.Embedding(30, 4)
    emb.load_state_dict({"weight": O.procedural_uniform((30, 4), 1.0, 32)})
    tr = Trainer({"coarse": m.to(DEV), "t": emb.to(DEV)}, args, use_graph=False)
    rays, ts = O.synthetic_rays(128, seed=33)
    target = torch.rand(128, 3, generator=torch.Generator().manual_seed(35))
    depth = data.DepthBank(rays_d, depths, ts_d, batch_size=96, seed=2).next_batch()
    loss = tr.step(rays.to(DEV), ts.to(DEV), target.to(DEV), depth=depth)
    assert math.isfinite(loss.item())
