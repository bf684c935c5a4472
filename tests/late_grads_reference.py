"""Host references for the fixed-order sky and embedding gradients (include/satrender.h: the ``*_det`` entry points).

* ``scratch_words`` / ``scratch_views``: the scratch layout the header documents, written out a second time.
* ``reduce_sky`` / ``reduce_emb``: the two ordered reductions, emulated with sequential fp32 adds (numpy float32 arithmetic is IEEE
  round-to-nearest, one rounding per add, no FMA) -- the device results must equal them bit for bit.
* ``sky_grads_fp64`` / ``emb_grads_fp64``: the gradients themselves from the kernels' inputs in fp64, with the sum of the absolute values
  of their terms for a first-order error bound.  A "term" is one product of the fully expanded sum: e.g. g_w2[c, k] is the sum over
  rays r and j of dz[r, c] * w1[k, j] * sun[r, j] plus dz[r, c] * b1[k] (the hidden pre-activation is itself a rounded sum: its error is
  relative to ITS terms, not to its value).
* ``late_bound``: (n_blocks + 32) * 2^-24 * sum|terms| -- a chain of n_blocks fp32 adds behind the in-block sums (16 + 1 adds, or a 6-level
  lane tree), with a few roundings per term."""
import numpy as np
import torch

SKY_RAYS = 32   # rays per sky block (csrc/ray_ops.hip kSkyRays)
HEAD_WORDS = 4  # the arrival counter, padded to 16 bytes


def sky_row(hidden):
    return 7 * hidden + 3


def sky_blocks(n_rays):
    return (n_rays + SKY_RAYS - 1) // SKY_RAYS


def scratch_words(n_sky, hidden, n_emb, tau):
    """4-byte words of a scratch with a sky part for ``n_sky`` rays and an embedding part for ``n_emb`` rays (0 = that part is absent)."""
    return HEAD_WORDS + sky_blocks(n_sky) * sky_row(hidden) + n_emb * tau + n_emb


def scratch_bytes(n_rays, hidden, tau):
    """What sr_late_grad_scratch_bytes returns: the scratch of a tail launch."""
    return 4 * scratch_words(n_rays, hidden, n_rays, tau)


def scratch_views(scratch, n_sky, hidden, n_emb, tau):
    """(counter word as int, sky_part (blocks, 7 hidden + 3), emb_part (n_emb, tau), first (n_emb,) int32) of a float32 scratch tensor, on the host."""
    s = scratch.detach().cpu()
    a = HEAD_WORDS
    b = a + sky_blocks(n_sky) * sky_row(hidden)
    c = b + n_emb * tau
    return (int(s[:1].view(torch.int32).item()), s[a:b].view(sky_blocks(n_sky), sky_row(hidden)).numpy().copy(),
            s[b:c].view(n_emb, max(tau, 1)).numpy().copy() if n_emb else np.zeros((0, max(tau, 1)), np.float32),
            s[c:c + n_emb].view(torch.int32).numpy().copy())


def split_sky(flat, hidden):
    """A (7 hidden + 3,) vector in the row's order -> (g_w1 (hidden, 3), g_b1 (hidden,), g_w2 (3, hidden), g_b2 (3,))."""
    h = hidden
    return flat[:3 * h].reshape(h, 3), flat[3 * h:4 * h], flat[4 * h:7 * h].reshape(3, h), flat[7 * h:]


def join_sky(g_w1, g_b1, g_w2, g_b2):
    return np.concatenate([np.asarray(t).reshape(-1) for t in (g_w1, g_b1, g_w2, g_b2)])


def reduce_sky(part, g0):
    """acc = 0.0f; for b in order: acc += part[b][i]; g[i] = g0[i] + acc -- all in fp32."""
    part, acc = np.asarray(part, np.float32), np.zeros(part.shape[1], np.float32)
    for b in range(part.shape[0]):
        acc = acc + part[b]
    assert acc.dtype == np.float32
    return np.asarray(g0, np.float32) + acc


def reduce_emb(part, ts, g0):
    """acc[row] = 0.0f; for r in increasing order: acc[ts[r]] += part[r]; g[row] = g0[row] + acc[row] for the rows some ray names; others untouched."""
    part, g = np.asarray(part, np.float32), np.array(g0, np.float32, copy=True)
    acc = {}
    for r, row in enumerate(np.asarray(ts).tolist()):
        acc[row] = acc.get(row, np.zeros(part.shape[1], np.float32)) + part[r]
    for row, a in acc.items():
        assert a.dtype == np.float32
        g[row] = g[row] + a
    return g


def first_of_row(ts):
    """1 where no earlier ray names ray r's row."""
    seen, out = set(), []
    for row in np.asarray(ts).tolist():
        out.append(0 if row in seen else 1)
        seen.add(row)
    return np.array(out, np.int32)


def hidden_preacts_fp64(sun, w1, b1):
    return sun.double() @ w1.double().t() + b1.double()


def sky_grads_fp64(sun, w1, b1, w2, sky, d_sky):
    """(gradient, sum of |terms|), both (7 hidden + 3,) fp64 numpy in the row's order, of the sky head sigmoid(w2 relu(w1 sun + b1) + b2)
    given its output ``sky`` and the output's gradient ``d_sky``."""
    sun, w1, b1, w2, sky, d_sky = (t.detach().cpu().double() for t in (sun, w1, b1, w2, sky, d_sky))
    dz = d_sky * sky * (1.0 - sky)                                  # (n, 3)
    h = sun @ w1.t() + b1                                           # (n, hidden)
    habs = sun.abs() @ w1.abs().t() + b1.abs()                      # the pre-activation's own terms
    mask = (h > 0).double()
    dh = (dz @ w2) * mask
    dhabs = (dz.abs() @ w2.abs()) * mask
    g = join_sky((dh.t() @ sun).numpy(), dh.sum(0).numpy(), (dz.t() @ (h * mask)).numpy(), dz.sum(0).numpy())
    t = join_sky((dhabs.t() @ sun.abs()).numpy(), dhabs.sum(0).numpy(), (dz.abs().t() @ (habs * mask)).numpy(), dz.abs().sum(0).numpy())
    return g, t


def emb_grads_fp64(d_t, ts, n_rows):
    """(gradient, sum of |terms|), both (n_rows, tau) fp64 numpy: g[ts[r]] += sum_j d_t[r, j]."""
    d = d_t.detach().cpu().double()
    ts = ts.detach().cpu().long()
    g = torch.zeros(n_rows, d.shape[-1], dtype=torch.float64).index_add_(0, ts, d.sum(1))
    t = torch.zeros(n_rows, d.shape[-1], dtype=torch.float64).index_add_(0, ts, d.abs().sum(1))
    return g.numpy(), t.numpy()


def late_bound(n_rays, terms):
    return (sky_blocks(n_rays) + 32) * 2.0 ** -24 * np.asarray(terms, np.float64)
