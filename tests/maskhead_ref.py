"""TEST INFRASTRUCTURE ONLY -- the rule of include/tmr_maskhead.h restated in
float64 numpy, and the seeded draws the mask-head tests share."""
import math

import numpy as np
import torch


def _erf(x):  # float64 on the CPU
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def mask_head(src, hyper, W1, b1, g, beta, eps, W2, b2, size):
    """src [N,h*w,256], hyper [N,32], W1 [256,64,2,2], W2 [64,32,2,2] ->
    masks [N,4h,4w], float64.  Non-finite values propagate as IEEE gives them
    (a non-finite src row turns that pixel's 16 values NaN)."""
    h, w = size
    src, hyper, W1, b1, g, beta, W2, b2 = (np.asarray(a, np.float64) for a in (src, hyper, W1, b1, g, beta, W2, b2))
    N = src.shape[0]
    assert src.shape == (N, h * w, W1.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        # u[n][p][k][l][o]; a row of a matrix product depends on its own row of the left factor
        # only, so a non-finite src row stays with its pixel
        C, c1, c2 = W1.shape[0], W1.shape[1], W2.shape[1]
        u = (src.reshape(-1, C) @ W1.transpose(0, 2, 3, 1).reshape(C, 4 * c1)).reshape(N, h * w, 2, 2, c1) + b1
        mu = u.mean(-1, keepdims=True)
        s = ((u - mu) ** 2).mean(-1, keepdims=True)
        a = gelu(g * ((u - mu) / np.sqrt(s + float(eps))) + beta)
        t = gelu((a.reshape(-1, c1) @ W2.transpose(0, 2, 3, 1).reshape(c1, 4 * c2)).reshape(N, -1, c2) + b2)
        v = (t @ hyper[:, :, None])[..., 0]  # [N][(p, k, l, m, j)]
    # mask[n][4y + 2k + m][4x + 2l + j]
    v = v.reshape(N, h, w, 2, 2, 2, 2).transpose(0, 1, 3, 5, 2, 4, 6)  # n y k m x l j
    return np.ascontiguousarray(v.reshape(N, 4 * h, 4 * w))


def normwise(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    return float(np.abs(got[ok] - ref[ok]).max() / np.abs(ref[ok]).max())


def weights(seed, dim=256):
    """Seeded output_upscaling weights: ConvTranspose2d-like uniform ranges,
    biases and LayerNorm parameters away from their 0 / 1 defaults."""
    rng = np.random.default_rng(seed)
    c1, c2 = dim // 4, dim // 8
    k1, k2 = 1.0 / math.sqrt(c1 * 4), 1.0 / math.sqrt(c2 * 4)
    return {
        "W1": rng.uniform(-k1, k1, (dim, c1, 2, 2)).astype(np.float32),
        "b1": rng.uniform(-k1, k1, c1).astype(np.float32),
        "g": rng.uniform(0.5, 1.5, c1).astype(np.float32),
        "beta": rng.uniform(-0.5, 0.5, c1).astype(np.float32),
        "eps": 1e-6,
        "W2": rng.uniform(-k2, k2, (c1, c2, 2, 2)).astype(np.float32),
        "b2": rng.uniform(-k2, k2, c2).astype(np.float32),
    }


def windowed_src(rng, N, h, w, dim=256, amp=3.0):
    """The fixture's kind of draw: amp * noise inside a random window of 2-3
    cells per side (clipped to the plane) per prompt, zero outside."""
    src = np.zeros((N, h, w, dim), np.float32)
    for n in range(N):
        hh, ww = min(h, int(rng.integers(2, 4))), min(w, int(rng.integers(2, 4)))
        y0, x0 = int(rng.integers(0, h - hh + 1)), int(rng.integers(0, w - ww + 1))
        src[n, y0:y0 + hh, x0:x0 + ww] = amp * rng.standard_normal((hh, ww, dim)).astype(np.float32)
    return src.reshape(N, h * w, dim)


def ref_of(wt, src, hyper, size):
    return mask_head(src, hyper, wt["W1"], wt["b1"], wt["g"], wt["beta"], wt["eps"], wt["W2"], wt["b2"], size)


# ---------------------------------------------------------------- torch side
# A decoder of the reference's structure (attribute and state-dict names as
# the reference's MaskDecoder), for the tests that need a module to wrap.
from torch import nn  # noqa: E402


class LayerNorm2d(nn.Module):
    def __init__(self, c, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.eps = eps

    def forward(self, x):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return self.weight[:, None, None] * ((x - u) / torch.sqrt(s + self.eps)) + self.bias[:, None, None]


class MLP(nn.Module):
    def __init__(self, cin, hidden, cout, n):
        super().__init__()
        dims = [cin] + [hidden] * (n - 1) + [cout]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i < len(self.layers) - 1:
                x = torch.relu(x)
        return x


class Replay(nn.Module):
    """A transformer stand-in that returns recorded (hs, src)."""

    def __init__(self, hs, src):
        super().__init__()
        self.hs, self.src, self.calls = hs, src, 0

    def forward(self, src, pos_src, tokens):
        assert src.shape[0] == tokens.shape[0] == self.hs.shape[0] and pos_src.shape == src.shape
        self.calls += 1
        return self.hs, self.src


class Decoder(nn.Module):
    """The stock decoder: structure, and the stock torch mask head."""

    def __init__(self, dim=256, transformer=None, iou_hidden=32, gelu=None, tokens=4):
        super().__init__()
        gelu = gelu or nn.GELU
        self.transformer_dim = dim
        self.transformer = transformer if transformer is not None else nn.Identity()
        self.iou_token = nn.Embedding(1, dim)
        self.num_mask_tokens = tokens
        self.mask_tokens = nn.Embedding(tokens, dim)
        self.output_upscaling = nn.Sequential(nn.ConvTranspose2d(dim, dim // 4, kernel_size=2, stride=2),
                                              LayerNorm2d(dim // 4), gelu(),
                                              nn.ConvTranspose2d(dim // 4, dim // 8, kernel_size=2, stride=2), gelu())
        self.output_hypernetworks_mlps = nn.ModuleList(MLP(dim, dim, dim // 8, 3) for _ in range(tokens))
        self.iou_prediction_head = MLP(dim, iou_hidden, tokens, 3)

    def stock_head(self, hs, src, size):
        """What the stock module computes after the transformer: all four
        masks, then the argmax selection.  Returns (masks [N,1,4h,4w], iou [N,1], ids)."""
        b, (h, w) = src.shape[0], size
        x = self.output_upscaling(src.transpose(1, 2).reshape(b, self.transformer_dim, h, w))
        hyper = torch.stack([self.output_hypernetworks_mlps[i](hs[:, 1 + i]) for i in range(self.num_mask_tokens)], 1)
        masks = (hyper @ x.view(b, x.shape[1], -1)).view(b, -1, 4 * h, 4 * w)
        iou = self.iou_prediction_head(hs[:, 0])
        ids = torch.argmax(iou, 1)
        ar = torch.arange(b, device=ids.device)
        return masks[ar, ids][:, None], iou[ar, ids][:, None], ids

    def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings,
                multimask_output=False):
        tokens = torch.cat([self.iou_token.weight, self.mask_tokens.weight], 0)
        tokens = torch.cat((tokens.unsqueeze(0).expand(sparse_prompt_embeddings.size(0), -1, -1),
                            sparse_prompt_embeddings), 1)
        src = torch.repeat_interleave(image_embeddings, tokens.shape[0], 0) + dense_prompt_embeddings
        pos = torch.repeat_interleave(image_pe, tokens.shape[0], 0)
        hs, out = self.transformer(src, pos, tokens)
        return self.stock_head(hs, out, tuple(src.shape[2:]))[:2]


def set_upscaling(up, wt):
    with torch.no_grad():
        for p, k in ((up[0].weight, "W1"), (up[0].bias, "b1"), (up[1].weight, "g"), (up[1].bias, "beta"),
                     (up[3].weight, "W2"), (up[3].bias, "b2")):
            p.copy_(torch.from_numpy(np.asarray(wt[k])))
    up[1].eps = float(wt["eps"])
    return up


def fixture_weights(g):
    up = "sd_output_upscaling."
    return {"W1": g[up + "0.weight"], "b1": g[up + "0.bias"], "g": g[up + "1.weight"], "beta": g[up + "1.bias"],
            "eps": float(g["eps"]), "W2": g[up + "3.weight"], "b2": g[up + "3.bias"]}


def decoder_from_fixture(g, hs, src):
    """The fixture's decoder (tests/golden/maskhead.npz) around a replay of (hs, src)."""
    dec = Decoder(transformer=Replay(hs, src))
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32)) for k in list(g.keys()) if k.startswith("sd_")}
    missing, extra = dec.load_state_dict(sd, strict=False)
    assert not missing and not extra, (missing, extra)
    dec.output_upscaling[1].eps = float(g["eps"])
    return dec.eval()
