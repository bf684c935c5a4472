"""The geometry (trunk + sigma) variants of the generated forward cores (csrc/gen/fwd_core.py / fwd_core512.py with heads=False ->
csrc/mlp_fwd_core_a*g.inc, mlp_fwd512_core_a*g.inc, written by the build; git holds their digests), after the pattern of
tests/test_fwd_core.py: the committed digests are current and the build writes exactly the pinned text, the
default arguments still emit the full cores byte for byte, and each geometry stream -- executed on stream_common.LaneModel against the
ONE packed forward stream, whose feats rows it jumps over -- leaves in SIG what the emulator's sigma is (under the bound test_fwd_core.py
holds the full cores' sigma to) and, lane for lane and bit for bit, what the full stream leaves there on the same weights and inputs.
A planted fault (the jump taken out) must not pass silently: the model names the rule, or SIG differs."""
import copy
import functools
import inspect
import os
import re

import numpy as np
import pytest

from satnerf_amd import packing
from tests import test_fwd_core as F

ROOT = F.ROOT
CSRC = os.path.join(ROOT, "satnerf_amd", "csrc")
WIDTHS = {256: ("fwd_core", "Core", "Machine", "mlp_fwd_core", F.test_instruction_stream_computes_the_forward_pass),
          512: ("fwd_core512", "Core512", "Machine512", "mlp_fwd512_core", F.test_width512_core_stream_computes_the_forward_pass)}


def _bound(feat):
    """the relative bound tests/test_fwd_core.py applies to the outputs (sigma among them) of this width's full core.  That file keeps it
    as a literal in the assert, not as a name, and is not edited here, so it is read from the test's source text rather than copied: brittle
    against a respelling of that line, and loud when it happens (the set must hold exactly one number)."""
    (b,) = set(re.findall(r"assert err < ([0-9.e-]+), \(name, err\)", inspect.getsource(WIDTHS[feat][4])))
    return float(b)


@functools.lru_cache(maxsize=None)
def _run(feat, tau, heads, jump=True):
    """the lane model after the stream of (feat, tau): full core or geometry core on the same packed stream, points and aux fragments.
    jump=False: the planted fault, the geometry stream with its source jump taken out of the instruction list and of the core."""
    mod, cls, machine, _, _ = WIDTHS[feat]
    g = F._gen(mod)
    auxs = g.aux_steps(tau)
    core = getattr(g, cls)(auxs, heads=heads)
    em, xyz, outputs = F._reference_tile(feat, tau, bf16=True, **({"l0_split": True} if feat == 256 else {}))
    bits = g.bf16_bits(em.stream.reshape(-1, 64, 8).astype(np.float32))
    if feat == 256:  # fc_net.0's 16 pieces: the kernel prologue writes them into the ring
        bits = np.concatenate([g.bf16_bits(g.l0_pieces(em.l0.astype(np.float32))), bits])
    stream_bits = (bits[:, :, 0::2] | (bits[:, :, 1::2] << 16)).astype(np.uint32)
    if not jump:
        core = copy.copy(core)
        at = [i for i, x in enumerate(core.ins) if x.op == "voff" and x.a]
        assert len(at) == 1 and core.ins[at[0]].a == (1 + core.SRC_JUMP[1],)
        core.ins = list(core.ins)
        core.ins[at[0]] = copy.copy(core.ins[at[0]])
        core.ins[at[0]].a = ()
        core.SRC_JUMP = None
    m = getattr(g, machine)(core, stream_bits)
    if feat == 256:
        for s, frag in enumerate(g.l0_b_frags(xyz.astype(np.float32))):
            m.v[g.L0B + 4 * s:g.L0B + 4 * s + 4] = g.f32_to_frag(frag)
        aux_at = g.AUX
    else:
        for k in range(32):
            m.v[g.X + 4 * k:g.X + 4 * k + 4] = g.f32_to_frag(em.saved["a"][0][k])
        aux_at = g.IN_AUX
    for a in range(auxs):
        m.v[aux_at + 4 * a:aux_at + 4 * a + 4] = g.f32_to_frag(em.saved["aux"][a])
    m.run()
    return g, core, m, outputs


@pytest.mark.parametrize("auxs", [1, 2])
@pytest.mark.parametrize("feat", [256, 512])
def test_committed_digests_of_the_geometry_streams_are_current(feat, auxs):
    """the text of the geometry streams is not in git, its digests are (csrc/gen/variant_streams.sha256): what the generator emits today
    has the committed digest, carries the name its kernel shell includes, and a file already in csrc/ (a built tree) is that text"""
    import hashlib

    mod, cls, _, stem, _ = WIDTHS[feat]
    g = F._gen(mod)
    name = f"{stem}_a{auxs}g.inc"
    want = getattr(g, cls)(auxs, heads=False).inc_file()
    assert g.STEM == stem and name in g.variant_files(getattr(g, cls), stem)
    assert g.read_digests()[name] == hashlib.sha256(want.encode()).hexdigest(), f"re-run satnerf_amd/csrc/gen/{mod}.py"
    with open(os.path.join(CSRC, "mlp_fwd2.inc" if feat == 256 else "mlp_fwd512g.inc")) as f:
        assert f'"{name}"' in f.read()
    if os.path.exists(os.path.join(CSRC, name)):
        with open(os.path.join(CSRC, name)) as f:
            assert f.read() == want, "a stale generated file: run build()"


def test_the_build_writes_the_pinned_streams_and_refuses_others(tmp_path, monkeypatch):
    """``generate_streams`` of the entry module: writes the four files where the kernels include them, leaves files with the committed
    digest alone, rewrites an edited one, and fails when the generators do not write what is pinned"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("graft_entry_under_test", os.path.join(ROOT, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    os.symlink(os.path.join(CSRC, "gen"), tmp_path / "gen")
    monkeypatch.setattr(entry, "CSRC", str(tmp_path))
    entry.generate_streams()
    names = sorted(n for n in os.listdir(tmp_path) if n != "gen")
    pins = F._gen("fwd_core").read_digests()
    assert names == sorted(pins) == sorted(f"{WIDTHS[w][3]}_a{a}g.inc" for w in WIDTHS for a in (1, 2))
    assert all(F._gen("fwd_core").file_digest(str(tmp_path / n)) == pins[n] for n in names)
    stamps = {n: os.stat(tmp_path / n).st_mtime_ns for n in names}
    entry.generate_streams()
    assert stamps == {n: os.stat(tmp_path / n).st_mtime_ns for n in names}
    with open(tmp_path / names[-1], "a") as f:
        f.write("// edited\n")
    entry.generate_streams()
    assert F._gen("fwd_core").file_digest(str(tmp_path / names[-1])) == pins[names[-1]]
    # a pin file that names other digests: the build stops
    import sys

    with open(tmp_path / "other.sha256", "w") as f:
        f.writelines(f"{'0' * 64}  {n}\n" for n in names)
    monkeypatch.setattr(sys.modules["stream_common"], "DIGESTS", str(tmp_path / "other.sha256"))
    with pytest.raises(RuntimeError, match="variant_streams.sha256 pins"):
        entry.generate_streams()


@pytest.mark.parametrize("auxs", [1, 2])
@pytest.mark.parametrize("feat", [256, 512])
def test_default_arguments_still_emit_the_full_cores(feat, auxs):
    mod, cls, _, stem, _ = WIDTHS[feat]
    C = getattr(F._gen(mod), cls)
    for save in (0, 8):
        with open(os.path.join(CSRC, f"{stem}_a{auxs}{'s8' if save else ''}.inc")) as f:
            text = f.read()
        assert text == C(auxs, save=save).inc_file() == C(auxs, save=save, heads=True).inc_file()


@pytest.mark.parametrize("tau", [4, 16])
@pytest.mark.parametrize("feat", [256, 512])
def test_geometry_stream_computes_sigma(feat, tau):
    g, core, m, outputs = _run(feat, tau, heads=False)
    full = _run(feat, tau, heads=True)
    assert core.stats["mfma"] < full[1].stats["mfma"] and [t.name for t in core.tiles][-2:] == [f"L7.{core.MT - 1}", "sigma.0"]
    sig = m.f(g.SIG).astype(np.float64)[:32]
    got = np.where(sig > 20, sig, np.log1p(np.exp(np.minimum(sig, 20))))
    want = outputs[1]
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    print(f"feat {feat} tau {tau}: sigma relative error {err:.3g} (bound {_bound(feat):g}), MFMAs {core.stats['mfma']} of {full[1].stats['mfma']}")
    assert err < _bound(feat), err
    assert np.array_equal(m.v[g.SIG], full[2].v[g.SIG]), "SIG differs from the full stream's, lane for lane"


@pytest.mark.parametrize("tau", [4, 16])
@pytest.mark.parametrize("feat", [256, 512])
def test_missing_feats_jump_does_not_pass_silently(feat, tau):
    """two plantings: the jump instruction alone reverted (the model must name the VOFF rule), and the jump taken out of instruction list
    and core alike, so that the model runs clean and the sigma tile multiplies feats' pieces (SIG must differ)"""
    mod, cls, machine, _, _ = WIDTHS[feat]
    g, core, good, _ = _run(feat, tau, heads=False)
    c = copy.copy(core)
    c.ins = [x if not (x.op == "voff" and x.a) else type(x)("voff", (), x.text) for x in core.ins]
    assert [x.a for x in c.ins] != [x.a for x in core.ins]
    with pytest.raises(AssertionError, match=re.escape("VOFF does not address row j of the stream")):
        with np.errstate(all="ignore"):
            getattr(g, machine)(c, np.zeros((core.n_pieces + core.NW * core.SRC_JUMP[1], 64, 4), np.uint32)).run()
    bad = _run(feat, tau, heads=False, jump=False)[2]
    assert not np.array_equal(bad.v[g.SIG], good.v[g.SIG])


@pytest.mark.parametrize("tau", [4, 16])
@pytest.mark.parametrize("feat", [256, 512])
def test_jump_lands_on_the_sigma_pieces_of_the_packed_stream(feat, tau):
    """the source rows the sigma tile's ring rows are fed from hold, in packing.forward_maps, sigma_from_xyz.0's row and nothing else"""
    mod, cls, _, _, _ = WIDTHS[feat]
    g = F._gen(mod)
    core = getattr(g, cls)(g.aux_steps(tau), heads=False)
    maps = packing.forward_maps(feat, tau)
    pre = core.PRE_ROWS * core.NW  # ring pieces the kernel prologue writes: not part of the packed stream
    tile = core.tiles[-1]
    assert tile.name == "sigma.0" and tile.p0 % core.NW == 0 and tile.p0 // core.NW == core.SRC_JUMP[0]
    w_off, w_shape = maps["offsets"]["sigma_from_xyz.0.weight"]
    b_off, _ = maps["offsets"]["sigma_from_xyz.0.bias"]
    for k in range(tile.n):
        p = tile.p0 + k
        src = core.NW * core.src_row(p // core.NW) + p % core.NW - pre
        piece = maps["idx"][src * 512:(src + 1) * 512].reshape(2, 32, 8)  # [h, row, j]
        assert (piece[:, 1:] == -1).all(), k
        live = piece[:, 0][piece[:, 0] >= 0]
        if k < feat // 16:
            assert live.size == 16 and ((live >= w_off) & (live < w_off + w_shape[1])).all(), k
        else:
            assert set(live.tolist()) <= {b_off} and (k > feat // 16 or live.size == 1), k
    assert (tile.p0 + tile.n - pre) + core.NW * core.SRC_JUMP[1] <= maps["idx"].size // 512
