"""TEST INFRASTRUCTURE ONLY -- the rules of include/tmr_twoway.h and the whole
two-way transformer restated in float64 numpy (UNFOLDED, in the stock module's
order, and folded through the two rules), the seeded weights and draws the
two-way tests share, and a torch module of SAM's published structure with the
stock attribute names (for the tests that need a module to wrap)."""
import math

import numpy as np
import torch
from torch import nn

DIM, HEADS, SLOTS = 256, 8, 8
ATTN = ("q_proj", "k_proj", "v_proj", "out_proj")


def normwise(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    return float(np.abs(got[ok] - ref[ok]).max() / np.abs(ref[ok]).max())


# ---------------------------------------------------------------- weights
def weights(seed, depth=2, dim=DIM, mlp_dim=64, downsample=2, scale=1.0):
    """Seeded state dict (numpy fp32) of a TwoWayTransformer: matrices uniform
    in +-scale / sqrt(fan_in), biases in +-0.3 but never within 0.02 of 0,
    LayerNorm weights in [0.5, 1.5] but never within 0.02 of 1."""
    rng = np.random.default_rng(seed)
    sd = {}

    def away(lo, hi, n, centre):
        v = rng.uniform(lo, hi, n)
        near = np.abs(v - centre) < 0.02
        v[near] = centre + 0.02 * np.where(v[near] >= centre, 1.0, -1.0)
        return v.astype(np.float32)

    def linear(name, cin, cout):
        k = scale / math.sqrt(cin)
        sd[name + ".weight"] = rng.uniform(-k, k, (cout, cin)).astype(np.float32)
        sd[name + ".bias"] = away(-0.3, 0.3, cout, 0.0)

    def attention(name, inner):
        for p in ATTN[:3]:
            linear(f"{name}.{p}", dim, inner)
        linear(f"{name}.out_proj", inner, dim)

    def norm(name):
        sd[name + ".weight"] = away(0.5, 1.5, dim, 1.0)
        sd[name + ".bias"] = away(-0.5, 0.5, dim, 0.0)

    for i in range(depth):
        L = f"layers.{i}"
        attention(L + ".self_attn", dim)
        norm(L + ".norm1")
        attention(L + ".cross_attn_token_to_image", dim // downsample)
        norm(L + ".norm2")
        linear(L + ".mlp.lin1", dim, mlp_dim)
        linear(L + ".mlp.lin2", mlp_dim, dim)
        norm(L + ".norm3")
        norm(L + ".norm4")
        attention(L + ".cross_attn_image_to_token", dim // downsample)
    attention("final_attn_token_to_image", dim // downsample)
    norm("norm_final_attn")
    return sd


def depth_of(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("layers."))


# ---------------------------------------------------------------- the two rules
def softmax(s, axis):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(s - np.max(s, axis=axis, keepdims=True))  # np.max propagates NaN; inf - inf = NaN
        return e / e.sum(axis=axis, keepdims=True)


def pool_rule(keys, pe, qf, T):
    """keys [Nk,P,256], pe [P,256], qf [N,64,256] -> ctx [N,64,256], float64;
    absent rows (t >= T) 0."""
    keys, pe, qf = (np.asarray(a, np.float64) for a in (keys, pe, qf))
    N = qf.shape[0]
    out = np.zeros_like(qf)
    present = (np.arange(HEADS * SLOTS) % SLOTS) < T
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            k = keys[n if keys.shape[0] > 1 else 0]
            s = qf[n][present] @ (k + pe).T  # [rows, P]
            out[n][present] = np.einsum("jp,pc->jc", softmax(s, 1), k)  # plain loops: 0 * inf stays NaN
    return out


def layer_norm(x, g, b, eps):
    with np.errstate(invalid="ignore", over="ignore"):
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        return g * ((x - mu) / np.sqrt(var + eps)) + b


def update_rule(keys, pe, A, c, B, bo, g, beta, eps, T):
    """-> keys_out [N,P,256], float64."""
    keys, pe, A, c, B, bo, g, beta = (np.asarray(a, np.float64) for a in (keys, pe, A, c, B, bo, g, beta))
    N, P = A.shape[0], keys.shape[1]
    out = np.empty((N, P, DIM))
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            x = keys[n if keys.shape[0] > 1 else 0]
            s = (x + pe) @ A[n].T + c[n]  # [P, 64]
            s = s.reshape(P, HEADS, SLOTS)[:, :, :T]
            a = softmax(s, 2)
            y = bo + np.einsum("pht,htc->pc", a, B[n].reshape(HEADS, SLOTS, DIM)[:, :T])
            out[n] = layer_norm(x + y, g, beta, eps)
    return out


# ---------------------------------------------------------------- the transformer, float64
def _lin(sd, name, x):
    return x @ np.asarray(sd[name + ".weight"], np.float64).T + np.asarray(sd[name + ".bias"], np.float64)


def _heads(x):
    n, t, c = x.shape
    return x.reshape(n, t, HEADS, c // HEADS).transpose(0, 2, 1, 3)


def attention(sd, name, q, k, v):
    """The stock Attention.forward, unfolded."""
    q, k, v = _heads(_lin(sd, name + ".q_proj", q)), _heads(_lin(sd, name + ".k_proj", k)), \
        _heads(_lin(sd, name + ".v_proj", v))
    with np.errstate(invalid="ignore", over="ignore"):
        a = softmax(q @ k.transpose(0, 1, 3, 2) / math.sqrt(q.shape[-1]), -1)
        o = (a @ v).transpose(0, 2, 1, 3)
    return _lin(sd, name + ".out_proj", o.reshape(o.shape[0], o.shape[1], -1))


def _norm(sd, name, x, eps=1e-5):
    return layer_norm(x, np.asarray(sd[name + ".weight"], np.float64), np.asarray(sd[name + ".bias"], np.float64), eps)


def _tokens_front(sd, L, i, queries, pe_q):
    if i == 0:
        queries = attention(sd, L + ".self_attn", queries, queries, queries)
    else:
        q = queries + pe_q
        queries = queries + attention(sd, L + ".self_attn", q, q, queries)
    return _norm(sd, L + ".norm1", queries)


def _mlp(sd, L, queries):
    return _norm(sd, L + ".norm3", queries + _lin(sd, L + ".mlp.lin2", np.maximum(_lin(sd, L + ".mlp.lin1", queries), 0)))


def transformer(sd, image_embedding, image_pe, point_embedding):
    """The stock TwoWayTransformer.forward (activation ReLU), float64, unfolded.
    image_embedding, image_pe [N,256,h,w] -> (hs [N,T,256], keys [N,hw,256],
    keys after layer 0)."""
    e, pe, pt = (np.asarray(a, np.float64) for a in (image_embedding, image_pe, point_embedding))
    keys = e.reshape(e.shape[0], e.shape[1], -1).transpose(0, 2, 1)
    kpe = pe.reshape(pe.shape[0], pe.shape[1], -1).transpose(0, 2, 1)
    queries, keys0 = pt, None
    for i in range(depth_of(sd)):
        L = f"layers.{i}"
        queries = _tokens_front(sd, L, i, queries, pt)
        queries = _norm(sd, L + ".norm2", queries + attention(sd, L + ".cross_attn_token_to_image", queries + pt,
                                                              keys + kpe, keys))
        queries = _mlp(sd, L, queries)
        keys = _norm(sd, L + ".norm4", keys + attention(sd, L + ".cross_attn_image_to_token", keys + kpe, queries + pt,
                                                        queries))
        if i == 0:
            keys0 = keys
    queries = _norm(sd, "norm_final_attn", queries + attention(sd, "final_attn_token_to_image", queries + pt,
                                                               keys + kpe, keys))
    return queries, keys, keys0


def _rows(x):
    """[N,T,H,...] -> [N,64,...], row 8 h + t."""
    N, T, H = x.shape[:3]
    out = np.zeros((N, H, SLOTS) + x.shape[3:])
    out[:, :, :T] = np.swapaxes(x, 1, 2)
    return out.reshape((N, H * SLOTS) + x.shape[3:])


def fold_t2i(sd, name, q, drop_k_bias=True):
    """qf [N,64,256]; with drop_k_bias=False also the per-row constant the
    k_proj bias adds to every pixel's score (it cancels in the softmax)."""
    N, T, _ = q.shape
    W = lambda p: np.asarray(sd[f"{name}.{p}.weight"], np.float64)  # noqa: E731
    d = W("q_proj").shape[0] // HEADS
    qh = _lin(sd, name + ".q_proj", q).reshape(N, T, HEADS, d) / math.sqrt(d)
    qf = _rows(np.einsum("nthd,hdc->nthc", qh, W("k_proj").reshape(HEADS, d, -1)))
    if drop_k_bias:
        return qf
    return qf, _rows(np.einsum("nthd,hd->nth", qh, np.asarray(sd[name + ".k_proj.bias"], np.float64).reshape(HEADS, d)))


def unfold_ctx(sd, name, ctx, T):
    N = ctx.shape[0]
    Wv = np.asarray(sd[name + ".v_proj.weight"], np.float64)
    d = Wv.shape[0] // HEADS
    c = ctx.reshape(N, HEADS, SLOTS, -1)[:, :, :T]
    v = np.einsum("nhtc,hdc->nthd", c, Wv.reshape(HEADS, d, -1)) \
        + np.asarray(sd[name + ".v_proj.bias"], np.float64).reshape(HEADS, d)
    return _lin(sd, name + ".out_proj", v.reshape(N, T, HEADS * d))


def fold_i2t(sd, name, k_tok, v_tok):
    N, T, _ = k_tok.shape
    Wq = np.asarray(sd[name + ".q_proj.weight"], np.float64)
    d = Wq.shape[0] // HEADS
    kt = _lin(sd, name + ".k_proj", k_tok).reshape(N, T, HEADS, d) / math.sqrt(d)
    vt = _lin(sd, name + ".v_proj", v_tok).reshape(N, T, HEADS, d)
    A = np.einsum("nthd,hdc->nthc", kt, Wq.reshape(HEADS, d, -1))
    c = np.einsum("nthd,hd->nth", kt, np.asarray(sd[name + ".q_proj.bias"], np.float64).reshape(HEADS, d))
    B = np.einsum("nthd,chd->nthc", vt, np.asarray(sd[name + ".out_proj.weight"], np.float64).reshape(-1, HEADS, d))
    return _rows(A), _rows(c), _rows(B)


def transformer_folded(sd, image_embedding, image_pe, point_embedding, pool=pool_rule, update=update_rule):
    """The same forward through the two rules (image_pe [1,256,h,w] or one per
    prompt, all equal; image_embedding [1 or N, 256, h, w])."""
    e, pe, pt = (np.asarray(a, np.float64) for a in (image_embedding, image_pe, point_embedding))
    keys = e.reshape(e.shape[0], e.shape[1], -1).transpose(0, 2, 1)
    kpe = pe[0].reshape(pe.shape[1], -1).T
    T = pt.shape[1]
    queries, keys0 = pt, None
    f64 = lambda k: np.asarray(sd[k], np.float64)  # noqa: E731
    for i in range(depth_of(sd)):
        L = f"layers.{i}"
        queries = _tokens_front(sd, L, i, queries, pt)
        name = L + ".cross_attn_token_to_image"
        ctx = pool(keys, kpe, fold_t2i(sd, name, queries + pt), T)
        queries = _norm(sd, L + ".norm2", queries + unfold_ctx(sd, name, ctx, T))
        queries = _mlp(sd, L, queries)
        name = L + ".cross_attn_image_to_token"
        A, c, B = fold_i2t(sd, name, queries + pt, queries)
        keys = update(keys, kpe, A, c, B, f64(name + ".out_proj.bias"), f64(L + ".norm4.weight"),
                      f64(L + ".norm4.bias"), 1e-5, T)
        if i == 0:
            keys0 = keys
    name = "final_attn_token_to_image"
    ctx = pool(keys, kpe, fold_t2i(sd, name, queries + pt), T)
    queries = _norm(sd, "norm_final_attn", queries + unfold_ctx(sd, name, ctx, T))
    return queries, keys, keys0


# ---------------------------------------------------------------- draws for the kernel tests
def operands(seed, N, P, T, Nk, score_span=None):
    """fp32 operands of both kernels: keys, pe ~ N(0,1); qf, A scaled so the
    scores have unit-order spread (or span about +-score_span); rows t >= T of
    qf, A, c, B hold NaN: absent rows are never read."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    d = {"keys": f(Nk, P, DIM), "pe": f(P, DIM), "qf": f(N, 64, DIM) / 16, "A": f(N, 64, DIM) / 16,
         "c": f(N, 64), "B": f(N, 64, DIM), "bo": f(DIM) / 4,
         "g": rng.uniform(0.5, 1.5, DIM).astype(np.float32), "beta": rng.uniform(-0.5, 0.5, DIM).astype(np.float32)}
    if score_span is not None:  # sd of a score = |qf row| * sqrt 2; its extremes over P pixels ~ 3 sd
        d["qf"] = (d["qf"] * (score_span / 3.0 / (math.sqrt(2.0) * math.sqrt(DIM) / 16))).astype(np.float32)
    absent = (np.arange(64) % SLOTS) >= T
    for k in ("qf", "A", "c", "B"):
        d[k][:, absent] = np.nan
    return d


# ---------------------------------------------------------------- torch side
class Attention(nn.Module):
    def __init__(self, dim, heads, downsample=1):
        super().__init__()
        self.embedding_dim, self.internal_dim, self.num_heads = dim, dim // downsample, heads
        self.q_proj = nn.Linear(dim, self.internal_dim)
        self.k_proj = nn.Linear(dim, self.internal_dim)
        self.v_proj = nn.Linear(dim, self.internal_dim)
        self.out_proj = nn.Linear(self.internal_dim, dim)

    def _split(self, x):
        b, n, c = x.shape
        return x.reshape(b, n, self.num_heads, c // self.num_heads).transpose(1, 2)

    def forward(self, q, k, v):
        q, k, v = self._split(self.q_proj(q)), self._split(self.k_proj(k)), self._split(self.v_proj(v))
        a = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(q.shape[-1]), dim=-1)
        o = (a @ v).transpose(1, 2)
        return self.out_proj(o.reshape(o.shape[0], o.shape[1], -1))


class MLPBlock(nn.Module):
    def __init__(self, dim, mlp_dim):
        super().__init__()
        self.lin1, self.lin2, self.act = nn.Linear(dim, mlp_dim), nn.Linear(mlp_dim, dim), nn.ReLU()

    def forward(self, x):
        return self.lin2(self.act(self.lin1(x)))


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_dim, downsample, skip_first_layer_pe):
        super().__init__()
        self.self_attn = Attention(dim, heads)
        self.norm1 = nn.LayerNorm(dim)
        self.cross_attn_token_to_image = Attention(dim, heads, downsample)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MLPBlock(dim, mlp_dim)
        self.norm3 = nn.LayerNorm(dim)
        self.norm4 = nn.LayerNorm(dim)
        self.cross_attn_image_to_token = Attention(dim, heads, downsample)
        self.skip_first_layer_pe = skip_first_layer_pe

    def forward(self, queries, keys, query_pe, key_pe):
        if self.skip_first_layer_pe:
            queries = self.self_attn(q=queries, k=queries, v=queries)
        else:
            q = queries + query_pe
            queries = queries + self.self_attn(q=q, k=q, v=queries)
        queries = self.norm1(queries)
        queries = self.norm2(queries + self.cross_attn_token_to_image(q=queries + query_pe, k=keys + key_pe, v=keys))
        queries = self.norm3(queries + self.mlp(queries))
        keys = self.norm4(keys + self.cross_attn_image_to_token(q=keys + key_pe, k=queries + query_pe, v=queries))
        return queries, keys


class TwoWayTransformer(nn.Module):
    """SAM's two-way transformer (ReLU MLP), stock attribute names."""

    def __init__(self, depth=2, dim=DIM, heads=HEADS, mlp_dim=64, downsample=2):
        super().__init__()
        self.depth, self.embedding_dim, self.num_heads, self.mlp_dim = depth, dim, heads, mlp_dim
        self.layers = nn.ModuleList(Block(dim, heads, mlp_dim, downsample, i == 0) for i in range(depth))
        self.final_attn_token_to_image = Attention(dim, heads, downsample)
        self.norm_final_attn = nn.LayerNorm(dim)
        self.calls = 0

    def forward(self, image_embedding, image_pe, point_embedding):
        self.calls += 1
        keys = image_embedding.flatten(2).permute(0, 2, 1)
        key_pe = image_pe.flatten(2).permute(0, 2, 1)
        queries = point_embedding
        for layer in self.layers:
            queries, keys = layer(queries, keys, point_embedding, key_pe)
        q = queries + point_embedding
        queries = self.norm_final_attn(queries + self.final_attn_token_to_image(q=q, k=keys + key_pe, v=keys))
        return queries, keys


def module(sd, **kw):
    """The torch stand-in with the state dict ``sd`` (numpy) loaded."""
    kw.setdefault("depth", depth_of(sd))
    kw.setdefault("mlp_dim", sd["layers.0.mlp.lin1.weight"].shape[0])
    kw.setdefault("downsample", DIM // sd["final_attn_token_to_image.q_proj.weight"].shape[0])
    tr = TwoWayTransformer(**kw)
    tr.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    return tr.eval()
