"""GPU-resident ray bank + on-device batch sampler.

Replaces ``DataLoader(train_dataset, shuffle=True, num_workers=4, batch_size=B, pin_memory=True)`` (main.py:96-110) over the
``(sum HW, 11)`` ray tensor ``SatelliteDataset`` builds (datasets/satellite.py:160-216, items ``{"rays": (11,), "rgbs": (3,),
"ts": (1,)}``, :347-350).  At > 1 M rays/s a per-item ``__getitem__`` + collate + H2D copy is two orders of magnitude too
slow; here the whole bank lives in HBM (45 B/ray: a 100 M-ray scene is 4.5 GB of 288 GB), an epoch is one ``randperm`` on the
device and a batch is one row gather.  Same sampling law as the DataLoader: every ray exactly once per epoch, in random order,
the last short batch dropped (``drop_last``) or kept.  Ranks draw disjoint strided shares of each epoch's permutation.
"""
from __future__ import annotations

import math

import torch


class RayBank:
    def __init__(self, rays, rgbs, ts, batch_size, seed=0, rank=0, world_size=1, drop_last=True):
        if not (rays.is_cuda and rgbs.is_cuda and ts.is_cuda):
            raise ValueError("RayBank tensors must already be on the GPU")
        n = rays.shape[0]
        if rgbs.shape[0] != n or ts.reshape(-1).shape[0] != n:
            raise ValueError("rays / rgbs / ts disagree on the number of rays")
        self.rays, self.rgbs, self.ts = rays.contiguous().float(), rgbs.contiguous().float(), ts.reshape(-1).contiguous().long()
        self.batch_size, self.rank, self.world, self.drop_last = batch_size, rank, world_size, drop_last
        self.gen = torch.Generator(device=rays.device)
        self.gen.manual_seed(seed)  # same seed on every rank: the ranks slice ONE permutation
        self.epoch, self._perm, self._pos = -1, None, 0

    def __len__(self):
        share = (self.rays.shape[0] - self.rank + self.world - 1) // self.world
        return share // self.batch_size if self.drop_last else (share + self.batch_size - 1) // self.batch_size

    def _new_epoch(self):
        self.epoch += 1
        perm = torch.randperm(self.rays.shape[0], device=self.rays.device, generator=self.gen)
        self._perm, self._pos = perm[self.rank::self.world], 0

    def next_indices(self):
        if self._perm is None or self._pos + (self.batch_size if self.drop_last else 1) > self._perm.numel():
            self._new_epoch()
        idx = self._perm[self._pos:self._pos + self.batch_size]
        self._pos += self.batch_size
        return idx

    # ---- in-graph sampler: the captured training step gathers its own batch (no host work between replays) ----------------------
    def graph_source(self):
        """(epoch index buffer (batches * B,) int64, cursor zeros(4) float32, batches) for ``ops.gather_batch(..., cursor=...)`` inside a
        captured step: the launch takes batch cursor[0] of the buffer and advances the cursor; ``graph_advance()`` after every
        replay keeps the host in step and reshuffles the buffer IN PLACE when an epoch ends.  Needs drop_last (full batches)."""
        if not self.drop_last:
            raise ValueError("the in-graph sampler serves full batches only (drop_last=True)")
        if getattr(self, "_gperm", None) is None:
            self._gbatches = len(self)
            if self._gbatches < 1:
                raise ValueError("the bank holds less than one batch")
            self._gperm = torch.empty(self._gbatches * self.batch_size, dtype=torch.int64, device=self.rays.device)
            self._gcursor = torch.zeros(4, dtype=torch.float32, device=self.rays.device)
            self.graph_reset()
        return self._gperm, self._gcursor, self._gbatches

    def graph_reset(self):
        """Start a fresh epoch at batch 0 (also after the capture's warm-up passes moved the cursor)."""
        self._new_epoch()
        self._gperm.copy_(self._perm[:self._gperm.numel()])
        self._gcursor.zero_()
        self._gpos = 0

    def graph_advance(self):
        """Host mirror of the device cursor: call once per replay; the next epoch's shuffle is written when the last batch is out."""
        self._gpos += 1
        if self._gpos == self._gbatches:
            self._new_epoch()
            self._gperm.copy_(self._perm[:self._gperm.numel()])  # stream-ordered after the replay that used the old epoch
            self._gpos = 0

    def gather(self, idx, out=None):
        """Rows ``idx`` -> (rays (B,11), ts (B,), rgbs (B,3)) on the device; ``out`` = three preallocated tensors of exactly that
        size to gather into (e.g. the static inputs of a captured hipGraph -- no intermediate copy)."""
        from . import ops

        if out is not None and out[0].shape[0] != idx.numel():
            raise ValueError(f"gather target holds {out[0].shape[0]} rays but the batch has {idx.numel()}")
        return ops.gather_batch(self.rays, self.rgbs, self.ts, idx.contiguous(), out)

    def next_batch(self, out=None):
        """The next batch of the shuffled epoch (``gather`` of ``next_indices``); a short last batch (drop_last=False) that does
        not fit ``out`` is returned in fresh tensors."""
        idx = self.next_indices()
        if out is not None and out[0].shape[0] != idx.numel():
            out = None
        return self.gather(idx, out)


class DepthBank(RayBank):
    """Ray bank of the depth-supervision dataset (``SatelliteDataset_depth``, datasets/satellite_depth.py: items
    ``{"rays": (11,), "depths": (2,) = [target depth, weight], "ts": (1,)}``; main.py:103-109 gives it its own shuffled
    DataLoader).  Batches come out as (rays (B,11), ts (B,), depths (B,3)) with a zero third column -- the gather kernel
    moves 3-float targets -- which is what ``Trainer.step(..., depth=...)`` takes."""

    def __init__(self, rays, depths, ts, batch_size, **kw):
        if depths.dim() != 2 or depths.shape[1] != 2:
            raise ValueError("depths must be (N, 2) = [target depth, weight]")
        super().__init__(rays, torch.cat([depths.float(), torch.zeros_like(depths[:, :1], dtype=torch.float32)], 1), ts, batch_size, **kw)


def sun_direction(sun_elevation_deg, sun_azimuth_deg):
    """Unit sun vector of one image (``SatelliteDataset.get_sun_dirs``, datasets/satellite.py:232-244)."""
    import math

    el, az = math.radians(float(sun_elevation_deg)), math.radians(float(sun_azimuth_deg))
    return torch.tensor([math.sin(az) * math.cos(el), math.cos(az) * math.cos(el), math.sin(el)], dtype=torch.float32)


def rays_from_cache(cached_rays, center, scene_range, sun_elevation_deg, sun_azimuth_deg, device=None):
    """The (HW, 11) fp32 ray block of one image from the reference's ``<cache_dir>/<img_id>.data`` file (``torch.save`` of the
    (HW, 8) ECEF rays ``get_rays`` produced; datasets/satellite.py:185-196): scene normalisation of origin / near / far
    (``normalize_rays``, :218-227) and the per-image sun direction appended (:199-211).  ``cached_rays`` = a path or the
    loaded tensor; arithmetic in the cache's own dtype before the final cast, like the reference.  Host-side data plumbing
    for ``RayBank``: the RPC localisation that writes the cache is not rebuilt."""
    rays = torch.load(cached_rays) if isinstance(cached_rays, (str, bytes)) or hasattr(cached_rays, "__fspath__") else cached_rays
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError(f"cached rays must be (HW, 8), got {tuple(rays.shape)}")
    rays = rays.clone()
    for c in range(3):
        rays[:, c] -= center[c]
        rays[:, c] /= scene_range
    rays[:, 6] /= scene_range
    rays[:, 7] /= scene_range
    sun = sun_direction(sun_elevation_deg, sun_azimuth_deg).to(rays.dtype).expand(rays.shape[0], 3)
    out = torch.hstack([rays, sun]).type(torch.float32)
    return out if device is None else out.to(device)


def rescale_rpc(rpc, alpha):
    """``sat_utils.rescale_rpc`` (sat_utils.py:44-57) on an "rpcm"-format dict: the camera of the image resized by ``alpha``."""
    out = dict(rpc)
    for k in ("row_scale", "col_scale", "row_offset", "col_offset"):
        out[k] = float(rpc[k]) * float(alpha)
    return out


def rays_from_rpc(rpc, height, width, min_alt, max_alt, center, scene_range, sun_elevation_deg, sun_azimuth_deg, device="cuda",
                  img_downscale=1.0, cache_path=None):
    """The (H*W, 11) ray block of one image straight from its RPC camera, on the GPU (``SatelliteDataset.load_data``,
    datasets/satellite.py:185-211, for an image without a ``.data`` cache): ``get_rays`` (:18-65) on the pixel grid of the
    down-scaled image, ``normalize_rays``, sun direction.  ``rpc`` = the JSON's "rpc" dict (rpcm format); ``height`` / ``width``
    = the FULL-resolution size stored in the JSON (the reference divides them by ``img_downscale`` itself, :191-192).
    ``cache_path``: also write the reference-compatible ``<cache_dir>/<img_id>.data`` file (torch.save of the (H*W, 8) rays)."""
    import os

    from . import ops

    h, w = int(height // img_downscale), int(width // img_downscale)
    rays, cache = ops.rpc_rays(rescale_rpc(rpc, 1.0 / img_downscale), w, h, min_alt, max_alt, center, scene_range, sun_elevation_deg,
                               sun_azimuth_deg, device, want_cache=cache_path is not None)
    if cache_path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(cache_path)), exist_ok=True)
        torch.save(cache.cpu(), cache_path)
    return rays


def _ortho_grid(grid):
    """(xoff, yoff, xsize, ysize, resolution) of a DSM grid as ``dsm.grid_from_roi`` returns it, checked."""
    vals = list(grid)
    if len(vals) != 5:
        raise ValueError(f"grid must hold (xoff, yoff, xsize, ysize, resolution), got {len(vals)} values")
    xoff, yoff, xsize, ysize, r = float(vals[0]), float(vals[1]), int(vals[2]), int(vals[3]), float(vals[4])
    if xsize < 1 or ysize < 1 or not r > 0:
        raise ValueError(f"zero-size DSM grid {tuple(vals)}")
    return xoff, yoff, xsize, ysize, r


def ortho_rays(grid, zone, min_alt, max_alt, center, scene_range, sun_d, device="cuda", out=None, return_latlon=False):
    """The (ysize * xsize, 11) fp32 ray block of a nadir camera over a DSM grid, on the GPU (csrc/ortho.hip):
    one ray straight down through the centre of every cell, row-major with row 0 at the top (``dsm.DSM``'s layout), so
    ``x.view(ysize, xsize, -1)`` of any per-ray output is its ortho image.  It is ``get_rays`` + ``normalize_rays``
    (datasets/satellite.py:18-65,218-227) with the RPC localisation replaced by the inverse UTM projection of the cell centre.

    ``grid`` = (xoff, yoff, xsize, ysize, resolution), e.g. ``dsm.grid_from_roi(roi)``; ``zone`` 1..60 or e.g. "17R" (false northing 0
    in both hemispheres, as everywhere here); ``min_alt`` < ``max_alt`` the altitude bounds of the scene; ``center`` (3,) /
    ``scene_range`` its ECEF normalisation; ``sun_d`` the (3,) sun direction every ray carries (``data.sun_direction``).  The origin sits
    at ``max_alt`` and is normalised in fp64 before its one rounding to fp32; near = 0, far = (max_alt - min_alt) / scene_range, so depth
    t means altitude max_alt - t * scene_range.  ``out``: a (ysize * xsize, >=11) fp32 device tensor whose columns 0..10 are written
    (e.g. a wider image buffer).  With ``return_latlon`` the result is (rays, latlon (ysize * xsize, 2) fp64 (lat, lon) degrees)."""
    from . import dsm, ops

    xoff, yoff, xsize, ysize, r = _ortho_grid(grid)
    dev = torch.device(device)
    if dev.type != "cuda" or (out is not None and not (torch.is_tensor(out) and out.is_cuda)):
        raise ValueError("ortho_rays runs on the GPU: satnerf_amd has no CPU path")
    if not float(min_alt) < float(max_alt):
        raise ValueError(f"need min_alt < max_alt, got {min_alt} and {max_alt}")
    if not float(scene_range) > 0:
        raise ValueError(f"scene_range must be > 0, got {scene_range}")
    sun = [float(v) for v in (sun_d.tolist() if hasattr(sun_d, "tolist") else sun_d)]
    if len(sun) != 3:
        raise ValueError(f"sun_d must hold 3 values, got {len(sun)}")
    ctr = [float(v) for v in (center.tolist() if hasattr(center, "tolist") else center)]
    rays, latlon = ops.ortho_rays(xoff, yoff, r, xsize, ysize, dsm._zone_number(zone), min_alt, max_alt, ctr, scene_range, sun, dev, out=out,
                                  want_latlon=return_latlon)
    rays = rays[:, :11]  # a wider ``out`` keeps its other columns to itself
    return (rays, latlon) if return_latlon else rays


def sun_rays(rays, depth, center, scene_range, max_alt, sun_d=None, bias=None, n_samples=None, out=None, return_valid=False,
             return_latlonalt=False):
    """The (N, 11) fp32 block of rays from rendered surface points towards the sun, on the GPU (csrc/sun_rays.hip, DESIGN.md section
    7.14).  Row i starts at ``P = o + d * depth[i]`` of primary ray ``rays[i]`` and runs along the sun vector -- the call's ``sun_d``
    (east, north, up; 3 values, not necessarily a unit vector) or, with ``sun_d=None``, the ray's own columns 8:11 -- turned into the
    east / north / up frame of P's geodetic position, i.e. into the scene's normalised ECEF frame.  near = the bias, far = where the ray
    reaches ``max_alt`` (metres) on the local tangent plane, at least near; columns 8:11 carry the sun vector as given.  Rendering these
    rays and keeping ``transparency[:, -1]`` is what ``rendering.render_sun_visibility`` does.

    ``center`` (3,) / ``scene_range``: the scene's ECEF normalisation.  ``bias`` keeps a ray from starting inside the surface it leaves:
    ``None`` = one sample interval of the primary ray, (far - near) / ``n_samples`` (which is then required); a float = an absolute
    distance in scene units.  The default is a derived quantity, not a tuned one: nobody has evaluated it on a trained scene.
    far grows as 1 / sin(elevation) and is not capped, so the samples of a very low sun thin out accordingly.

    A ray whose depth or surface point is not finite, or whose sun vector is zero, not finite or at or below the horizon, is invalid:
    its row is the finite zero-length ray [o, d, 0, 0, sun].  ``out``: an (N, >=11) fp32 device tensor whose columns 0..10 are written.
    Returns the rays, followed by ``valid`` (N,) bool with ``return_valid`` and ``latlonalt`` (3, N) fp64 (lat, lon degrees, alt metres
    of the surface points; ``rendering.latlonalt_from_depth``'s bits) with ``return_latlonalt``."""
    from . import ops

    if not (torch.is_tensor(rays) and rays.is_cuda and torch.is_tensor(depth) and depth.is_cuda) or (
            out is not None and not (torch.is_tensor(out) and out.is_cuda)):
        raise ValueError("sun_rays runs on the GPU: satnerf_amd has no CPU path")
    if rays.dim() != 2 or rays.shape[1] < 11:
        raise ValueError(f"rays must be (N, 11) with the sun direction in columns 8:11, got {tuple(rays.shape)}")
    if depth.numel() != rays.shape[0]:
        raise ValueError(f"depth must hold one value per ray ({rays.shape[0]}), got {tuple(depth.shape)}")
    if not float(scene_range) > 0:
        raise ValueError(f"scene_range must be > 0, got {scene_range}")
    if bias is None:
        if n_samples is None or int(n_samples) < 1:
            raise ValueError("bias=None means one sample interval of the primary ray: pass n_samples (>= 1), or an absolute bias")
        bias_abs, bias_rel = 0.0, 1.0 / int(n_samples)
    else:
        bias_abs, bias_rel = float(bias), 0.0
        if not (math.isfinite(bias_abs) and bias_abs >= 0):
            raise ValueError(f"bias must be finite and >= 0, got {bias}")
    sun = None
    if sun_d is not None:
        sun = [float(v) for v in (sun_d.tolist() if hasattr(sun_d, "tolist") else sun_d)]
        if len(sun) != 3:
            raise ValueError(f"sun_d must hold 3 values, got {len(sun)}")
    ctr = [float(v) for v in (center.tolist() if hasattr(center, "tolist") else center)]
    r32 = rays if rays.dtype == torch.float32 and rays.stride(1) == 1 else rays.float().contiguous()
    with torch.cuda.device(rays.device):
        sr, valid, lla = ops.sun_rays(r32, depth.reshape(-1).float().contiguous(), ctr, scene_range, max_alt, sun, bias_abs, bias_rel, out=out,
                                      want_latlonalt=return_latlonalt)
    res = (sr[:, :11],)  # a wider ``out`` keeps its other columns to itself
    if return_valid:
        res += (valid.bool(),)
    if return_latlonalt:
        res += (lla,)
    return res if len(res) > 1 else res[0]


def read_scene_loc(root_dir):
    """(center (3,) fp32 tensor, scene_range float) from ``root_dir/scene.loc`` as ``SatelliteDataset.__init__`` loads them
    (datasets/satellite.py:108-110): both rounded to fp32 (``scene_range`` is the fp32 maximum of the three scales, returned as a
    Python float of that value).  The file is required: the reference writes it in ``init_scaling_params``, which cannot serialise
    its own float32 values; here ``init_scaling_params(root_dir)`` writes it, and only when asked to."""
    import json
    import os

    path = os.path.join(root_dir, "scene.loc")
    if not os.path.exists(path):
        raise FileNotFoundError(f"Could not find {path}: the scene's normalisation (X/Y/Z_offset and X/Y/Z_scale of the ECEF bounds) is "
                                "required; write it with the scene's dataset tools or data.init_scaling_params (it is not computed here)")
    with open(path) as f:
        d = json.load(f)
    center = torch.tensor([float(d["X_offset"]), float(d["Y_offset"]), float(d["Z_offset"])])
    scene_range = torch.max(torch.tensor([float(d["X_scale"]), float(d["Y_scale"]), float(d["Z_scale"])]))
    return center, float(scene_range)


def scene_bounds(images, img_downscale=1.0, device="cuda", names=None, return_per_image=False):
    """The scene normalisation ``SatelliteDataset.init_scaling_params`` computes (datasets/satellite.py:135-156), on the GPU.

    ``images``: the per-image JSON dicts (``rpc`` in rpcm format, ``height``, ``width``, ``min_alt``, ``max_alt``); per image the grid
    is ``int(height // s) x int(width // s)`` under ``rescale_rpc(rpc, 1 / s)`` (:142-146), and one ``sr_rpc_scene_bounds`` launch
    writes the ECEF bounds of its rays' near and far points into its row of an (n_images, 6) table; the host reads that table and the
    per-image counts of non-finite pixels back in one copy.  An image whose down-scaled grid is empty adds no point, as the
    reference's meshgrid yields no ray for it.  The scene's extremes then go through ``sat_utils.rpc_scaling_params`` in float32
    (sat_utils.py:30-37): scale = (max - min) / 2, offset = min + scale.  Returns {"X_scale", "X_offset", "Y_scale", "Y_offset",
    "Z_scale", "Z_offset"} as Python floats holding those fp32 values; with ``return_per_image`` also the (n_images, 6) fp32 numpy
    table [xmin, xmax, ymin, ymax, zmin, zmax] (+inf / -inf in the row of an empty image).  An image with a non-finite pixel raises
    ``ValueError`` naming it (``names``: per-image labels, e.g. the JSON paths) and its count ``n_bad``."""
    import numpy as np

    from . import ops

    n_img = len(images)
    if n_img < 1:
        raise ValueError("no images")
    dev = torch.device(device)
    s = float(img_downscale)
    # one buffer, so one copy back: 6 fp32 bounds per image, then one int64 count per image (6 n int32 words is a multiple of 8 bytes)
    host = torch.zeros(8 * n_img, dtype=torch.int32)
    host[:6 * n_img].view(torch.float32).view(n_img, 6).copy_(torch.tensor([math.inf, -math.inf] * 3))
    raw = host.to(dev)
    bounds, n_bad = raw[:6 * n_img].view(torch.float32).view(n_img, 6), raw[6 * n_img:].view(torch.int64)
    sizes = []
    for k, d in enumerate(images):
        h, w = int(d["height"] // s), int(d["width"] // s)
        sizes.append(h * w)
        if h < 1 or w < 1:
            continue  # an empty grid: no ray, and no launch (the ABI wants at least one pixel)
        ops.rpc_scene_bounds(rescale_rpc(d["rpc"], 1.0 / s), w, h, float(d["min_alt"]), float(d["max_alt"]), dev, out=bounds[k],
                             n_bad=n_bad[k:k + 1])
    host = raw.cpu()  # the one device-to-host copy
    per_image = host[:6 * n_img].view(torch.float32).view(n_img, 6).numpy()
    bad = host[6 * n_img:].view(torch.int64).numpy()
    for k in range(n_img):
        if bad[k] > 0:
            name = names[k] if names is not None else f"image {k}"
            raise ValueError(f"{name}: n_bad = {int(bad[k])} of its {sizes[k]} pixels have a non-finite ray (RPC localisation or ECEF "
                             "point); scene bounds are undefined")
    lo, hi = per_image[:, 0::2].min(0), per_image[:, 1::2].max(0)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError(f"no pixels: every image's grid is empty at img_downscale {img_downscale}")
    out = {}
    for a, axis in enumerate("XYZ"):
        scale = (np.float32(hi[a]) - np.float32(lo[a])) / 2
        offset = np.float32(lo[a]) + scale
        out[axis + "_scale"], out[axis + "_offset"] = float(np.float32(scale)), float(np.float32(offset))
    return (out, per_image) if return_per_image else out


def init_scaling_params(root_dir, img_downscale=1.0, device="cuda", overwrite=False):
    """Write ``root_dir/scene.loc`` from the RPC cameras of every ``*.json`` under ``root_dir``, as ``SatelliteDataset.
    init_scaling_params`` is meant to (datasets/satellite.py:135-158; the reference's own ``json.dump`` refuses its float32 values):
    ``scene_bounds`` of those images, written with ``json.dump(..., indent=2)`` under the reference's six keys.  Returns what
    ``read_scene_loc(root_dir)`` returns.  ``FileExistsError`` if the file exists and ``overwrite`` is false; a JSON without an "rpc"
    field raises ``ValueError`` naming it."""
    import glob
    import json
    import os

    path = os.path.join(root_dir, "scene.loc")
    if os.path.exists(path) and not overwrite:
        raise FileExistsError(f"{path} exists (pass overwrite=True to replace it)")
    files = sorted(glob.glob("{}/*.json".format(root_dir)))
    if not files:
        raise FileNotFoundError(f"no *.json under {root_dir}")
    images = []
    for p in files:
        with open(p) as f:
            d = json.load(f)
        if not isinstance(d, dict) or "rpc" not in d:
            raise ValueError("No 'rpc' field was found in {}".format(p))
        images.append(d)
    loc = scene_bounds(images, img_downscale=img_downscale, device=device, names=files)
    with open(path, "w") as f:
        json.dump({k: loc[k] for k in ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")}, f, indent=2)
    return read_scene_loc(root_dir)


def _split_files(root_dir, name):
    import os

    with open(os.path.join(root_dir, name)) as f:
        return [os.path.join(root_dir, line.strip()) for line in f.read().split("\n") if line.strip()]


def _split_images(root_dir, split, img_downscale):
    """The images of a split in the order ``load_rays`` and ``load_colors`` share: ([(JSON dict, h, w)], ids) with the down-scaled size
    ``int(height // img_downscale)`` x ``int(width // img_downscale)`` (datasets/satellite.py:191-192).  ``"train"``: the ``train.txt``
    images, id = the line; ``"val"``: the first training image with id 0, then the ``test.txt`` images with ids n_train + k."""
    import json

    if split not in ("train", "val"):
        raise ValueError(f"split must be 'train' or 'val', got {split!r}")
    train = _split_files(root_dir, "train.txt")
    if split == "train":
        files, ids = train, list(range(len(train)))
    else:
        if not train:
            raise ValueError("train.txt lists no image")
        test = _split_files(root_dir, "test.txt")
        files, ids = [train[0]] + test, [0] + [len(train) + k for k in range(len(test))]
    metas = []
    for p in files:
        with open(p) as f:
            d = json.load(f)
        if "rpc" not in d:
            raise ValueError("No 'rpc' field was found in {}".format(p))
        metas.append((d, int(d["height"] // img_downscale), int(d["width"] // img_downscale)))
    return metas, ids


def load_rays(root_dir, split="train", img_downscale=1.0, device="cuda", cache_dir=None, create_scene_loc=False):
    """The rays ``SatelliteDataset(root_dir, img_dir, split, img_downscale, cache_dir)`` builds from a dataset directory, on the GPU.

    ``"train"`` (``load_train_split`` / ``load_data``, datasets/satellite.py:117-121, 160-216): returns (all_rays (N, 11) fp32 -- one
    preallocated tensor the images' blocks are written into --, all_ids (N,) int64 = the image's line in ``train.txt``, blank lines
    skipped, and a list of per-image (name, h, w, row_offset)).  ``"val"`` (``load_val_split``, :123-133): a list of per-image dicts
    {rays (h*w, 11), ts, src_id, h, w}: the first training image with ts 0, then the ``test.txt`` images with ts n_train + k;
    ``src_id`` is the file id of the JSON's "img".

    Rays come from ``sr_rpc_rays``.  With ``cache_dir`` an existing ``<cache_dir>/<img_id>.data`` is read through ``rays_from_cache``
    and a missing one is written (:185-196).  ``scene.loc`` is read with ``read_scene_loc``; when it is missing and
    ``create_scene_loc`` is true, ``init_scaling_params(root_dir, img_downscale)`` writes it first.

    Colours come from ``load_colors`` (or both at once from ``load_dataset``): image block k of the training split is rows ``row_offset ..
    row_offset + h * w`` in row-major pixel order (row ``i // w``, column ``i % w`` of the image resized to h x w), and ``load_colors``
    writes the same blocks of an (N, 3) colour tensor for ``RayBank(all_rays, rgbs, all_ids, batch_size)``."""
    import os

    from . import ops

    if split not in ("train", "val"):
        raise ValueError(f"split must be 'train' or 'val', got {split!r}")
    if create_scene_loc and not os.path.exists(os.path.join(root_dir, "scene.loc")):
        init_scaling_params(root_dir, img_downscale, device=device)
    center, scene_range = read_scene_loc(root_dir)
    metas, ids = _split_images(root_dir, split, img_downscale)
    dev = torch.device(device)
    s = float(img_downscale)

    def block(d, h, w, out):
        """One image's (h*w, 11) rays into ``out``."""
        img_id = os.path.splitext(os.path.basename(d["img"]))[0]
        cache_path = None if cache_dir is None else "{}/{}.data".format(cache_dir, img_id)
        if cache_path is not None and os.path.exists(cache_path):
            rays = rays_from_cache(cache_path, center, scene_range, float(d["sun_elevation"]), float(d["sun_azimuth"]))
            if rays.shape[0] != h * w:
                raise ValueError(f"{cache_path} holds {rays.shape[0]} rays but the image is {h} x {w} at img_downscale {img_downscale}")
            out.copy_(rays)
        elif h * w:
            _, cache = ops.rpc_rays(rescale_rpc(d["rpc"], 1.0 / s), w, h, float(d["min_alt"]), float(d["max_alt"]), center, scene_range,
                                    float(d["sun_elevation"]), float(d["sun_azimuth"]), dev, want_cache=cache_path is not None, out=out)
            if cache_path is not None:
                os.makedirs(os.path.dirname(os.path.abspath(cache_path)), exist_ok=True)
                torch.save(cache.cpu(), cache_path)
        return img_id

    if split == "train":
        counts = [h * w for _, h, w in metas]
        all_rays = torch.empty(sum(counts), 11, dtype=torch.float32, device=dev)
        all_ids = torch.repeat_interleave(torch.tensor(ids, dtype=torch.int64), torch.tensor(counts, dtype=torch.int64)).to(dev)
        index, off = [], 0
        for (d, h, w), n in zip(metas, counts):
            index.append((block(d, h, w, all_rays[off:off + n]), h, w, off))
            off += n
        return all_rays, all_ids, index
    out = []
    for (d, h, w), t in zip(metas, ids):
        rays = torch.empty(h * w, 11, dtype=torch.float32, device=dev)
        out.append({"rays": rays, "ts": t, "src_id": block(d, h, w, rays), "h": h, "w": w})
    return out


def _colors_on_device(op, what, image, h, w, device, out, layout, perturb=None):
    """``ops.<op>`` of a uint8 image (array or tensor, host or device) uploaded to ``device``, with that device current.  ``perturb``:
    (lut, rects, fills) for ``ops.blender_perturb`` to apply to the uploaded bytes first -- in place when the upload made a copy, into
    a new tensor when the bytes are still the caller's."""
    import contextlib

    import numpy as np

    from . import ops

    t = image if torch.is_tensor(image) else torch.from_numpy(np.require(np.asarray(image), requirements=["C", "W"]))
    if t.dtype != torch.uint8:
        raise ValueError(f"image must be uint8 ({what}), got {t.dtype}")
    dev = torch.device(device)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        u = t.to(dev).contiguous()
        if perturb is not None and any(p is not None for p in perturb):
            lut, rects, fills = perturb
            u = ops.blender_perturb(u, lut, rects, fills, layout=layout, out=u if u is not t else None)
        return getattr(ops, op)(u, int(h), int(w), out=out, layout=layout)


def colors_from_image(image, h, w, device="cuda", out=None, layout=None):
    """The (h * w, 3) fp32 colour rows of one 8-bit RGB image on the GPU, as ``load_tensor_from_rgb_geotiff`` (datasets/satellite.py:
    67-80) makes them: ``u8 / 255``, and the bicubic resize to h x w when that is not the image's own size.
    ``image``: a uint8 array or tensor, (H, W, 3) or (3, H, W), on the host or already on the device; the host uploads its 3 bytes per
    pixel and ``ops.image_colors`` does the rest.  ``out``: (h * w, 3) fp32 rows on ``device`` to write into; ``layout``: "hwc" / "chw"
    for an image whose shape reads both ways."""
    return _colors_on_device("image_colors", "8-bit colours", image, h, w, device, out, layout)


def _read_image_pillow(path):
    import numpy as np
    from PIL import Image

    with Image.open(path) as im:
        return np.asarray(im)


def load_colors(root_dir, img_dir, split="train", img_downscale=1.0, device="cuda", reader=None):
    """The colours ``SatelliteDataset(root_dir, img_dir, split, img_downscale)`` loads (``load_data``, datasets/satellite.py:160-216, through
    ``load_tensor_from_rgb_geotiff``, :67-80), on the GPU, in the order and sizes of ``load_rays``: image ``os.path.join(img_dir,
    d["img"])`` of every JSON of the split becomes h * w rows, h = int(height // img_downscale), w = int(width // img_downscale).

    ``"train"``: one (N, 3) fp32 tensor whose block k is rows ``row_offset .. row_offset + h * w`` of ``load_rays``'s index, written in
    place.  ``"val"``: a list of (h * w, 3) tensors in ``load_rays``'s order.  ``reader(path)`` returns the image as a uint8 array,
    (H, W, 3) or (3, H, W) (e.g. rasterio's ``f.read()``); the default opens the file with Pillow.  An image that is not 8-bit, does not
    have exactly three bands, or whose size is not the JSON's ``height`` x ``width`` raises ``ValueError`` naming the file -- the
    reference would pair such colours with the wrong rays.  An image whose down-scaled grid is empty is still read and checked, and
    adds no rows."""
    import os

    import numpy as np

    metas, _ = _split_images(root_dir, split, img_downscale)
    dev = torch.device(device)
    read = _read_image_pillow if reader is None else reader

    def block(d, h, w, out):
        """One image's (h*w, 3) colours into ``out``."""
        path = os.path.join(img_dir, d["img"])
        img = np.asarray(read(path))
        if img.dtype != np.uint8:
            raise ValueError(f"{path} is not an 8-bit image (its samples are {img.dtype}); 16-bit imagery is not supported")
        full = (int(d["height"]), int(d["width"]))
        shape = tuple(img.shape)
        if shape == full + (3,):
            layout = "hwc"
        elif shape == (3,) + full:
            layout = "chw"
        elif len(shape) != 3 or 3 not in (shape[0], shape[2]):
            raise ValueError(f"{path} does not have exactly three bands (its shape is {shape}); colours need an RGB image")
        else:
            size = shape[:2] if shape[2] == 3 else shape[1:]
            raise ValueError(f"{path} is {size[0]} x {size[1]} but its JSON says height x width = {full[0]} x {full[1]}: colours and "
                             "rays would not line up")
        if h * w:
            colors_from_image(img, h, w, dev, out=out, layout=layout)

    if split == "train":
        counts = [h * w for _, h, w in metas]
        all_rgbs = torch.empty(sum(counts), 3, dtype=torch.float32, device=dev)
        off = 0
        for (d, h, w), n in zip(metas, counts):
            block(d, h, w, all_rgbs[off:off + n])
            off += n
        return all_rgbs
    out = []
    for d, h, w in metas:
        out.append(torch.empty(h * w, 3, dtype=torch.float32, device=dev))
        block(d, h, w, out[-1])
    return out


def load_dataset(root_dir, img_dir, split="train", img_downscale=1.0, device="cuda", cache_dir=None, create_scene_loc=False, reader=None):
    """``load_rays`` and ``load_colors`` of one split: what ``SatelliteDataset(root_dir, img_dir, split, img_downscale, cache_dir)`` holds.
    ``"train"``: (all_rays (N, 11), all_rgbs (N, 3), all_ids (N,), index), ready for ``RayBank(all_rays, all_rgbs, all_ids, batch_size)``;
    ``"val"``: ``load_rays``'s per-image dicts with ``"rgbs"`` (h * w, 3) added, ready for ``evaluate_image``."""
    rays = load_rays(root_dir, split, img_downscale, device=device, cache_dir=cache_dir, create_scene_loc=create_scene_loc)
    rgbs = load_colors(root_dir, img_dir, split, img_downscale, device=device, reader=reader)
    if split == "train":
        all_rays, all_ids, index = rays
        return all_rays, rgbs, all_ids, index
    for v, c in zip(rays, rgbs):
        v["rgbs"] = c
    return rays


def blender_perturbation(seed, perturbation):
    """The host-side parameters of ``add_perturbation(img, perturbation, seed)`` (datasets/blender.py:61-79) for one frame: (lut, rects,
    fills), ready for ``ops.blender_perturb``.

    ``"color"``: s = uniform(0.8, 1.2, 3), b = uniform(-0.2, 0.2, 3), and a colour band's byte v becomes
    ``uint8(255 * clip(s * (v / 255.0) + b, 0, 1))`` in fp64 -- a function of the byte alone, so ``lut`` (4, 256) uint8 holds it exactly;
    the alpha row is ``uint8(255 * (v / 255.0))``, the identity.  ``"occ"``: left, top = randint(200, 400) twice, and rectangle i of ten
    spans columns left + 20 i .. left + 20 (i + 1) and rows top .. top + 200, both ends included, filled with
    ``choice(range(256), 3)`` of the generator seeded 10 * seed + i and alpha 255: ``rects`` (10, 4) int32 [x0, y0, x1, y1] and
    ``fills`` (10, 4) uint8.  A part that ``perturbation`` does not name is None.  Both parts reseed with ``seed``, as the reference
    does.  Unlike the reference, which seeds numpy's global generator, the draws come from ``np.random.RandomState`` objects (the same
    streams), and the process's global generator is left alone.  ``perturbation`` must be a subset of {"color", "occ"}."""
    import numpy as np

    if isinstance(perturbation, str) or not set(perturbation).issubset({"color", "occ"}):
        raise ValueError(f'Only "color" and "occ" perturbations are supported! (got {perturbation!r})')
    seed = int(seed)
    lut = rects = fills = None
    if "color" in perturbation:
        g = np.random.RandomState(seed)
        s, b = g.uniform(0.8, 1.2, size=3), g.uniform(-0.2, 0.2, size=3)
        x = np.repeat((np.arange(256) / 255.0)[:, None], 4, 1)
        x[:, :3] = np.clip(s * x[:, :3] + b, 0, 1)
        lut = np.ascontiguousarray((255 * x).astype(np.uint8).T)
    if "occ" in perturbation:
        g = np.random.RandomState(seed)
        left, top = g.randint(200, 400), g.randint(200, 400)
        rects, fills = np.empty((10, 4), np.int32), np.full((10, 4), 255, np.uint8)
        for i in range(10):
            rects[i] = left + 20 * i, top, left + 20 * (i + 1), top + 200
            fills[i, :3] = np.random.RandomState(10 * seed + i).choice(range(256), 3)
    return lut, rects, fills


def blender_colors_from_image(image, h, w, device="cuda", out=None, layout=None, perturb=None):
    """((h * w, 3) fp32 colours, (h * w,) bool valid_mask) of one 8-bit RGBA image on the GPU, as ``BlenderDataset`` makes them
    (datasets/blender.py:136-139,179-183): Pillow's Lanczos resize to h x w byte for byte, ``u8 / 255``, the blend onto white and
    ``alpha > 0``.  ``image``: a uint8 array or tensor, (H, W, 4) or (4, H, W), on the host or already on the
    device; the host uploads its 4 bytes per pixel and ``ops.blender_colors`` does the rest.  ``out``: (h * w, 3) fp32 rows on ``device``
    to write the colours into; ``layout``: "hwc" / "chw" for an image whose shape reads both ways.  ``perturb``: the (lut, rects, fills)
    of ``blender_perturbation``; the uploaded bytes then go through ``ops.blender_perturb`` before the resize, as the reference perturbs
    the full-size image (an image that was already on the device is left as it was)."""
    return _colors_on_device("blender_colors", "8-bit RGBA", image, h, w, device, out, layout, perturb)


def blender_rays(h, w, focal, c2w, near=2.0, far=6.0, device="cuda", out=None):
    """The (h * w, 8) fp32 rays [o, d, near, far] of one Blender frame on the GPU: ``get_ray_directions(h, w, K)`` and ``get_rays`` with
    ``read_meta``'s K (datasets/blender.py:12-59,104-112): fx = fy = focal, cx = w / 2, cy = h / 2.  ``c2w``: the frame's (3, 4)
    camera-to-world matrix.  ``out``: (h * w, 8) fp32 rows on ``device`` to write into."""
    import contextlib

    from . import ops

    dev = torch.device(device)
    with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
        return ops.pinhole_rays(h, w, focal, focal, w / 2, h / 2, c2w, near, far, out=out)


def load_blender(root_dir, split="train", img_wh=(400, 400), device="cuda", reader=None):
    """What ``BlenderDataset(root_dir, split, img_wh)`` holds (datasets/blender.py:82-209, ``perturbation=[]``), on the GPU.

    Reads ``transforms_{split.split('_')[-1]}.json``; focal = 0.5 * 800 / tan(0.5 * camera_angle_x) * (img_wh[0] / 800) in fp64, near 2,
    far 6; frame images are ``os.path.join(root_dir, frame["file_path"] + ".png")``, read through ``reader(path)`` -- a uint8 array,
    (H, W, 4) or (4, H, W) -- or Pillow.  Colours come from ``blender_colors_from_image``, rays from ``blender_rays``.

    ``"train"``: (all_rays (N, 8), all_rgbs (N, 3), all_ts (N,) int64); frame t's block is rows ``t h w .. (t + 1) h w`` in row-major
    pixel order with ts = t, written in place frame after frame (the reference's ``all_rays[:, :8]``, ``all_rgbs`` and
    ``all_rays[:, 8].long()``).  Any other split (``"val"``, ``"test"``, ``"test_train"``): a list of the reference's ``__getitem__``
    dicts {"rays" (h w, 8), "ts" (h w,) int64, "rgbs" (h w, 3), "c2w" (3, 4), "valid_mask" (h w,) bool}, one per frame; ``"val"`` stops
    after 8 frames (its ``__len__``), and ts is 0 except for ``"test_train"``, where frame idx != 0 gets idx.  An image that is not
    8-bit or does not have exactly four bands raises ``ValueError`` naming the file (the reference would blend with the blue channel as
    alpha); so does an ``img_wh`` that is not square (the reference's assert).  The layout is read off the shape: exactly one of the
    first and last axes must be 4, so a 4 x W x 4 array is refused as ambiguous; an array whose first axis is 4 is taken as (4, H, W)
    whatever its last axis (a (4, W, 3) array cannot be told from an RGBA image three pixels wide)."""
    return _load_blender(root_dir, (), split, img_wh, device, reader)


def load_blender_perturbed(root_dir, perturbation, split="train", img_wh=(400, 400), device="cuda", reader=None):
    """What ``BlenderDataset(root_dir, split, img_wh, perturbation)`` holds (datasets/blender.py:61-79,91-95,132-134,176-178,198-207), on
    the GPU: NeRF-W's "images in the wild" variant of a Blender scene.  ``perturbation``: a subset of {"color", "occ"}; empty, this is
    ``load_blender``, whose arguments, checks and return values it shares.

    ``"train"``: frame t != 0 is perturbed with seed t -- ``blender_perturbation(t, perturbation)`` applied by ``ops.blender_perturb`` to
    the full-size bytes, colour first, then the occluders, before the resize.  ``"test_train"``: frame idx != 0 is perturbed with seed
    idx, and with a non-empty ``perturbation`` every dict (frame 0's too) also carries ``"original_rgbs"`` and
    ``"original_valid_mask"`` of the unperturbed image.  ``"val"`` and ``"test"`` are never perturbed.  The draws do not touch numpy's
    global generator (``blender_perturbation``)."""
    blender_perturbation(0, perturbation)  # refuses an unknown name before anything is read
    return _load_blender(root_dir, tuple(perturbation), split, img_wh, device, reader)


def _load_blender(root_dir, perturbation, split, img_wh, device, reader):
    """``load_blender_perturbed``; ``load_blender`` is its ``perturbation=()``."""
    import json
    import math
    import os

    import numpy as np

    w, h = int(img_wh[0]), int(img_wh[1])
    if w != h:
        raise ValueError(f"img_wh must be square, as the reference requires (got {tuple(img_wh)})")
    which = split.rsplit("_", 1)[-1]  # "test_train" reads the training frames
    with open(os.path.join(root_dir, "transforms_" + which + ".json")) as f:
        meta = json.load(f)
    focal = (400.0 / math.tan(meta["camera_angle_x"] / 2)) * (w / 800)  # the 800-pixel focal length, then the scale to w, in that order
    near, far = 2.0, 6.0
    dev = torch.device(device)
    read = _read_image_pillow if reader is None else reader

    def block(frame, rays, rgbs, seed=0, original=False):
        """One frame's rays and colours into ``rays`` and ``rgbs``, perturbed with ``seed`` unless that is 0; returns (c2w, valid_mask),
        and with ``original`` also the unperturbed image's (rgbs, valid_mask)."""
        c2w = np.array(frame["transform_matrix"], dtype=np.float64)[:3, :4].astype(np.float32)
        path = os.path.join(root_dir, frame["file_path"] + ".png")
        img = np.asarray(read(path))
        if img.dtype != np.uint8:
            raise ValueError(f"{path} is not an 8-bit image (its samples are {img.dtype}); 16-bit imagery is not supported")
        first, last = img.ndim == 3 and img.shape[0] == 4, img.ndim == 3 and img.shape[2] == 4
        if not (first or last):
            raise ValueError(f"{path} does not have exactly four bands (its shape is {tuple(img.shape)}); the loader needs an RGBA image")
        if first and last:
            raise ValueError(f"{path} has shape {tuple(img.shape)}, which reads as (H, W, 4) and as (4, H, W): the loader cannot tell its "
                             "four bands from a side of four pixels")
        layout = "chw" if first else "hwc"
        perturb = blender_perturbation(seed, perturbation) if seed and perturbation else None
        _, mask = blender_colors_from_image(img, h, w, dev, out=rgbs, layout=layout, perturb=perturb)
        blender_rays(h, w, focal, c2w, near, far, dev, out=rays)
        if original:
            return c2w, mask, blender_colors_from_image(img, h, w, dev, layout=layout) if perturb else (rgbs.clone(), mask.clone())
        return c2w, mask

    frames = meta["frames"]
    n = h * w
    if split == "train":
        all_rays = torch.empty(len(frames) * n, 8, dtype=torch.float32, device=dev)
        all_rgbs = torch.empty(len(frames) * n, 3, dtype=torch.float32, device=dev)
        for t, frame in enumerate(frames):
            block(frame, all_rays[t * n:(t + 1) * n], all_rgbs[t * n:(t + 1) * n], seed=t)
        all_ts = torch.arange(len(frames), dtype=torch.int64, device=dev).repeat_interleave(n)
        return all_rays, all_rgbs, all_ts
    out = []
    for idx, frame in enumerate(frames[:8] if split == "val" else frames):
        rays = torch.empty(n, 8, dtype=torch.float32, device=dev)
        rgbs = torch.empty(n, 3, dtype=torch.float32, device=dev)
        t = idx if split == "test_train" and idx != 0 else 0
        extras = split == "test_train" and bool(perturbation)
        c2w, mask, *orig = block(frame, rays, rgbs, seed=t, original=extras)
        out.append({"rays": rays, "ts": torch.full((n,), t, dtype=torch.int64, device=dev), "rgbs": rgbs,
                    "c2w": torch.from_numpy(c2w).to(dev), "valid_mask": mask})
        if extras:
            out[-1]["original_rgbs"], out[-1]["original_valid_mask"] = orig[0]
    return out


def depth_supervision_from_keypoints(images, tie_points, center, scene_range, device="cuda", return_point_weights=False, names=None):
    """The depth-supervision data of ``SatelliteDataset_depth.load_depth_data`` (datasets/satellite_depth.py:51-129), on the GPU.

    ``images``: the per-image JSON dicts of the training split, in order (image t gets ``ts`` = t), each with ``rpc`` (rpcm format,
    full resolution), ``keypoints`` {``2d_coordinates`` (K, 2) = (col, row), ``pts3d_indices`` (K,)}, ``min_alt``, ``max_alt``,
    ``sun_elevation``, ``sun_azimuth``; ``tie_points``: (n_pts, 3) fp64 ECEF (pts3d.npy); ``center`` / ``scene_range``: from
    ``read_scene_loc``; ``names``: per-image labels for error messages (the JSON paths).  Returns (rays (N, 11), depths (N, 2) =
    [target depth, keypoint weight], ts (N,) int64) on ``device``, ready for ``DepthBank``; with ``return_point_weights`` also the
    per-tie-point error sums ``e`` and weights ``w`` (n_pts,).  The host only parses and uploads the tables once; every
    per-observation step runs in HIP.  Departures: an image without keypoints adds no rays but counts as a
    camera; indices outside pts3d and a zero or non-finite mean error raise ``ValueError``."""
    import math

    import numpy as np

    from . import ops

    pts = np.ascontiguousarray(np.asarray(tie_points, dtype=np.float64))
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"tie_points must be (n_pts, 3) ECEF points with n_pts >= 1, got {pts.shape}")
    n_pts, n_cams = pts.shape[0], len(images)
    if n_cams < 1:
        raise ValueError("no training images")
    colrows, idxs, counts = [], [], []
    for t, d in enumerate(images):
        name = names[t] if names is not None else f"image {t}"
        if "keypoints" not in d.keys():
            raise ValueError("No 'keypoints' field was found in {}".format(name))
        cr = np.asarray(d["keypoints"]["2d_coordinates"], dtype=np.float64).reshape(-1, 2)
        ix = np.asarray(d["keypoints"]["pts3d_indices"], dtype=np.int64).reshape(-1)
        if cr.shape[0] != ix.shape[0]:
            raise ValueError(f"{name}: {cr.shape[0]} keypoints but {ix.shape[0]} pts3d_indices")
        if ix.size and (ix.min() < 0 or ix.max() >= n_pts):
            raise ValueError(f"{name}: pts3d_indices must lie in 0..{n_pts - 1} (got {ix.min()}..{ix.max()})")
        colrows.append(cr), idxs.append(ix), counts.append(ix.size)
    n = int(sum(counts))
    dev = torch.device(device)
    with torch.cuda.device(dev):
        colrow = torch.from_numpy(np.concatenate(colrows)).to(dev)
        idx = torch.from_numpy(np.concatenate(idxs)).to(dev)
        ts = torch.repeat_interleave(torch.arange(n_cams, dtype=torch.int64), torch.tensor(counts, dtype=torch.int64)).to(dev)
        pts3d = torch.from_numpy(pts).to(dev)
        rays = torch.empty(n, 11, dtype=torch.float32, device=dev)
        err = torch.empty(n, dtype=torch.float32, device=dev)
        off = 0
        for d, k in zip(images, counts):
            if k:
                sl = slice(off, off + k)
                ops.rpc_rays_at(d["rpc"], colrow[sl], float(d["min_alt"]), float(d["max_alt"]), center, scene_range, float(d["sun_elevation"]),
                                float(d["sun_azimuth"]), out=rays[sl])
                ops.reprojection_errors(d["rpc"], colrow[sl], idx[sl], pts3d, out=err[sl])
            off += k
        e, w, e_mean = ops.keypoint_weights(idx, ts, err, n_pts, n_cams)
        depths = ops.tie_point_depths(rays, pts3d, idx, center, scene_range, w=w)
        em = e_mean.item()  # the one host synchronisation
    if not (math.isfinite(em) and em > 0):
        raise ValueError(f"the mean reprojection error over the tie points is {em}: the keypoint weights exp(-(e / e_mean)^2) are "
                         "undefined (no observed tie point, or non-finite errors)")
    return (rays, depths, ts, e, w) if return_point_weights else (rays, depths, ts)


def read_depth_dataset(root_dir):
    """(images, tie_points, center, scene_range, json_files) of a dataset directory as ``SatelliteDataset_depth`` reads them
    (datasets/satellite_depth.py:31-49): ``scene.loc``, the JSONs listed in ``train.txt`` (blank lines skipped) and ``pts3d.npy``."""
    import json
    import os

    import numpy as np

    center, scene_range = read_scene_loc(root_dir)
    with open(os.path.join(root_dir, "train.txt")) as f:
        json_files = [os.path.join(root_dir, line) for line in f.read().split("\n") if line.strip()]
    pts_path = root_dir + "/pts3d.npy"
    if not os.path.exists(pts_path):
        raise FileNotFoundError("Could not find {}".format(pts_path))
    tie_points = np.load(pts_path)
    images = []
    for p in json_files:
        with open(p) as f:
            images.append(json.load(f))
    return images, tie_points, center, scene_range, json_files


def load_depth_supervision(root_dir, device="cuda", return_point_weights=False):
    """``SatelliteDataset_depth(root_dir, img_dir, split="train")``'s ``all_rays``, ``all_depths`` and ``all_ids`` (datasets/
    satellite_depth.py:31-101) on the GPU, from ``scene.loc``, ``train.txt``, the training JSONs and ``pts3d.npy`` under
    ``root_dir`` -- no images and no ``img_dir``.  Returns what ``depth_supervision_from_keypoints`` returns (ts = the image's line
    in train.txt; blank lines are skipped)."""
    images, tie_points, center, scene_range, json_files = read_depth_dataset(root_dir)
    return depth_supervision_from_keypoints(images, tie_points, center, scene_range, device=device,
                                            return_point_weights=return_point_weights, names=json_files)


def synthetic_rays(n_rays, seed=20240628, n_images=19, far_lo=0.5, far_hi=1.0):
    """Synthetic sat-nerf ray batch for benchmarks (no dataset ships offline): origins U[-1,1]^3, unit directions, near = 0
    (datasets/satellite.py:60), far U[far_lo, far_hi] (scene-normalised, :225-226), one sun direction per synthetic image id
    from random (azimuth, elevation in [30, 80] deg) as in ``get_sun_dirs`` (:239-241), ts ~ randint(n_images).
    Returns (rays (N,11) fp32 on the CPU, ts (N,) int64)."""
    import math

    g = torch.Generator().manual_seed(seed)
    o = torch.rand(n_rays, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=1)
    far = far_lo + (far_hi - far_lo) * torch.rand(n_rays, 1, generator=g)
    az = torch.rand(n_images, generator=g) * 2 * math.pi
    el = math.radians(30) + torch.rand(n_images, generator=g) * math.radians(50)
    sun = torch.stack([torch.sin(az) * torch.cos(el), torch.cos(az) * torch.cos(el), torch.sin(el)], 1)
    ts = torch.randint(0, n_images, (n_rays,), generator=g)
    return torch.cat([o, d, torch.zeros(n_rays, 1), far, sun[ts]], 1).float(), ts


def default_args(**kw):
    """The ``args`` attributes the hot path reads, with the BASELINE configs[1] values (opt.py defaults except fc_units=256)."""
    from types import SimpleNamespace

    a = dict(model="sat-nerf", n_samples=64, n_importance=0, chunk=5120, noise_std=0.0, sc_lambda=0.0, ds_lambda=0.0, fc_layers=8,
             fc_units=256, t_embbeding_tau=4, t_embbeding_vocab=30)
    a.update(kw)
    return SimpleNamespace(**a)
