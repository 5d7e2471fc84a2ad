"""A tiny model with adapters whose merge is exact, for the model-level multi-LoRA tests: "adapter a on the device" then equals "the
oracle on the merged weights" up to summation order and the two extra roundings of the adapter arithmetic (tests/lora.py).

The oracle's synthetic wqkv / wo / w2 are snapped to the grid g = 2^-13 (integers |W| <= 283).  An adapter has A = a 2^-6 with integers
|a| <= 3, B = b 2^-(7 + log2 scale) with |b| <= 3 and a power-of-two scale, so scale B A = (b a) g: W + scale B A is an integer below 2^11
on the grid g -- exactly an fp16 matrix, which merged() asserts in float64.  A fused-qkv adapter is block diagonal as an exported PEFT
adapter is: A stacks the q, k and v factors, B holds each one's columns on its own rows."""
import numpy as np

from oracle import ref

GRID = 2.0 ** -13
TARGETS = ("attention.wqkv", "attention.wo", "feed_forward.w2")
PROMPT_LENS = (70, 3, 129, 1, 16, 33, 5, 64)
SLOTS = (-1, 0, 1, 2, 0, -1, 2, 1)
JOIN_LEN, JOIN_SLOT = 20, 1
# adapter id -> (fused wqkv rank as (q, k, v) parts or one dense rank, wo rank, w2 rank, scale); 0 = the target has no factors
ADAPTERS = {0: ((8, 8, 8), 8, 8, 1.0), 1: ((16, 16, 16), 16, 24, 2.0), 2: ((16,), 0, 16, 0.5)}
# (geometry, KV form) -> {adapter group: cap k of check_steps}; group -1 = the requests without an adapter.  1.5 x the observed worst error
# rounded up to the next 0.5: the figures are in tests/test_gpu_lora_model.py and profiles/lora_parity.jsonl
K_CAP = {
    ("mha", "fp16"): {-1: 0.5, 0: 1.0, 1: 0.5, 2: 1.0},
    ("gqa", "i8paged"): {-1: 0.5, 0: 1.0, 1: 1.0, 2: 1.5},
}


def make_desc(geom, kv):
    H, Hkv = {"mha": (4, 4), "gqa": (8, 2)}[geom]
    kw = {"fp16": dict(cache_quant_bit=0, cache_quant_group=1, cache_mode=0, page_size=0),
          "i8paged": dict(cache_quant_bit=8, cache_quant_group=8, cache_mode=1, page_size=16)}[kv]
    return ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=2, num_heads=H, num_kv_heads=Hkv, vocab_size=1024, max_position=512,
                         cache_layout=3, weight_quant_bit=0, weight_quant_group=128, **kw)


def shapes(desc):
    D = desc.hidden_dim // desc.num_heads
    nq, nkv = desc.num_heads * D, desc.num_kv_heads * D
    return {"attention.wqkv": (nq + 2 * nkv, desc.hidden_dim), "attention.wo": (desc.hidden_dim, nq),
            "feed_forward.w2": (desc.hidden_dim, desc.intermediate_dim)}, (nq, nkv, nkv)


def base_weights(desc, seed=1234):
    """{name: array} of the oracle's synthetic model with the three target matrices of every layer snapped to GRID"""
    rm = ref.RefModel(desc)
    rm.init_synthetic(seed)
    w = {}
    sh, _ = shapes(desc)
    for name in ref.tensor_names(desc):
        a = rm.get_tensor(name, np.float16)
        for t in TARGETS:
            if name.endswith(t + ".weight"):
                a = (np.round(a.astype(np.float64) / GRID) * GRID).astype(np.float16).reshape(sh[t])
        w[name] = a
    rm.close()
    return w


def make_adapter(desc, aid, seed=0, amp=3):
    """({tensor name: fp16 array}, scale) of adapter `aid`; amp: the integers' range (merged() checks that the merge stays exact)"""
    qkv, r_wo, r_w2, scale = ADAPTERS[aid]
    rng = np.random.RandomState(100 + 17 * aid + seed)
    sh, parts = shapes(desc)
    ub = 2.0 ** -(7 + int(np.log2(scale)))
    out = {}
    for l in range(desc.num_layers):
        for t, r in (("attention.wqkv", sum(qkv)), ("attention.wo", r_wo), ("feed_forward.w2", r_w2)):
            if not r:
                continue
            N, K = sh[t]
            a = rng.randint(-amp, amp + 1, size=(r, K))
            b = rng.randint(-amp, amp + 1, size=(N, r))
            if t == "attention.wqkv" and len(qkv) == 3:     # block diagonal: rows of q / k / v see their own ranks only
                mask = np.zeros((N, r), dtype=bool)
                n0 = j0 = 0
                for n, rr in zip(parts, qkv):
                    mask[n0:n0 + n, j0:j0 + rr] = True
                    n0, j0 = n0 + n, j0 + rr
                b = b * mask
            out[f"layers.{l}.{t}.lora_a"] = (a * 2.0 ** -6).astype(np.float16)
            out[f"layers.{l}.{t}.lora_b"] = (b * ub).astype(np.float16)
    return out, scale


def merged(weights, adapter, scale):
    """the base weights with W + scale B A in place of every adapted matrix; asserts that each is exactly an fp16 matrix"""
    w = dict(weights)
    for name, a in adapter.items():
        if not name.endswith(".lora_a"):
            continue
        stem = name[:-len(".lora_a")]
        b = adapter[stem + ".lora_b"]
        full = weights[stem + ".weight"].astype(np.float64) + float(scale) * (b.astype(np.float64) @ a.astype(np.float64))
        assert (full.astype(np.float16).astype(np.float64) == full).all(), ("merge is not exact", stem)
        assert (full != weights[stem + ".weight"].astype(np.float64)).mean() > 0.5, ("the adapter changes little", stem)
        w[stem + ".weight"] = full.astype(np.float16)
    return w


def oracle(desc, weights, kv_tokens):
    rm = ref.RefModel(desc)
    for k, v in weights.items():
        rm.set_tensor(k, v)
    rm.kv_alloc(kv_tokens)
    return rm


class Trace:
    """The run of the issue: a packed prefill of eight requests, three decode steps, one mixed step in which a new prompt joins.  One
    oracle per adapter plus the base runs every step whole (requests are independent); each request's rows come from its own oracle and
    the oracles' greedy tokens drive the next step."""

    def __init__(self, desc, seed=7, kv_tokens=1024):
        self.desc, self.kv_tokens = desc, kv_tokens
        rng = np.random.RandomState(seed)
        self.prompts = [rng.randint(3, desc.vocab_size, size=n) for n in PROMPT_LENS]
        self.join = rng.randint(3, desc.vocab_size, size=JOIN_LEN)
        self.weights = base_weights(desc)
        self.adapters = {a: make_adapter(desc, a) for a in ADAPTERS}
        self.oracles = {-1: oracle(desc, self.weights, kv_tokens)}
        for a, (t, s) in self.adapters.items():
            self.oracles[a] = oracle(desc, merged(self.weights, t, s), kv_tokens)

    def cache_plan(self, lens_total):
        from tests.test_gpu_model import plan_cache
        return plan_cache(self.desc, lens_total, self.kv_tokens)

    def steps(self):
        """yields (step arguments for make_step, slots [B]) and takes back nothing: the oracles' tokens are computed here"""
        n = len(self.prompts)
        lens = np.array([len(p) for p in self.prompts] + [JOIN_LEN])
        cache_idx, max_pages = self.cache_plan(lens + 6)
        slots = np.array(list(SLOTS), dtype=np.int32)
        tok = np.concatenate(self.prompts).astype(np.int64)
        seq_starts = np.concatenate([[0], np.cumsum(lens[:n])])
        start_pos = np.zeros(n, dtype=np.int64)
        for s in range(5):
            B = len(start_pos)
            dec = 0 if s == 0 else n
            args = (tok, seq_starts, start_pos, cache_idx[:B], dec, max_pages)
            want, alt = self.run_oracles(args, slots)
            yield s, args, slots, want, alt
            wtok, _ = ref.sample(want, top_k=1)
            start_pos = start_pos + (seq_starts[1:] - seq_starts[:-1])
            tok = wtok.astype(np.int64)
            seq_starts = np.arange(B + 1)
            if s == 3:   # the mixed step: eight decode rows, then the new prompt
                tok = np.concatenate([tok, self.join]).astype(np.int64)
                seq_starts = np.concatenate([seq_starts, [B + JOIN_LEN]])
                start_pos = np.concatenate([start_pos, [0]])
                slots = np.concatenate([slots, [JOIN_SLOT]]).astype(np.int32)

    def run_oracles(self, args, slots):
        from tests.parity import oracle_noise
        B = len(args[2])
        want = np.empty((B, self.desc.vocab_size), dtype=np.float32)
        alt = np.empty_like(want)
        for a, rm in self.oracles.items():
            rows = np.nonzero(slots == a)[0]
            st = ref.make_step(*args)
            w = ref.forward([rm], st)
            al = oracle_noise([rm], st)
            want[rows], alt[rows] = w[rows], al[rows]
        return want, alt


def group_results(res, slots_by_step, group):
    """the rows of adapter `group` out of per-step (got, want, gtok, wtok, glp, wlp, alt) tuples, in check_steps' form"""
    out = []
    for r, slots in zip(res, slots_by_step):
        rows = np.nonzero(slots == group)[0]
        out.append(tuple(x[rows] for x in r))
    return out


# ---------------------------------------------------------------------------------------------------------------
# what the adapter arithmetic's extra roundings are worth, without a device
# ---------------------------------------------------------------------------------------------------------------
def _f16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def _rms(h, skip, w, eps):
    r = _f16(h + skip) if skip is not None else h
    return _f16(r / np.sqrt((r * r).mean(-1, keepdims=True) + eps) * w), r


def numpy_forward(desc, W, prompt, lin):
    """The specification's forward for ONE request prefilled from position 0 with an fp16 KV cache, exact (float64)
    sums and the specification's fp16 roundings: last-token logits.  lin(name, x) is the layer linear `name` (wqkv / wo / w2) on rows x."""
    hd, H, Hkv = desc.hidden_dim, desc.num_heads, desc.num_kv_heads
    D, T = hd // H, len(prompt)
    half = D // 2

    def g(n):
        return W[n].astype(np.float64)

    h, pending = g("tok_embeddings.weight").reshape(-1, hd)[prompt], None
    ang = np.arange(T)[:, None] * desc.rope_theta ** (-np.arange(half) * 2.0 / D)
    c, s = np.cos(ang).astype(np.float32).astype(np.float64), np.sin(ang).astype(np.float32).astype(np.float64)
    causal = np.tril(np.ones((T, T))) > 0
    for l in range(desc.num_layers):
        xn, h = _rms(h, pending, g(f"layers.{l}.attention_norm.weight"), desc.norm_eps)
        qkv = lin(f"layers.{l}.attention.wqkv", xn).reshape(T, H + 2 * Hkv, D)
        x = qkv[:, :H + Hkv]
        a, b = x[..., :half].copy(), x[..., half:].copy()
        x[..., :half] = _f16(a * c[:, None] - b * s[:, None])
        x[..., half:] = _f16(b * c[:, None] + a * s[:, None])
        q, k, v = qkv[:, :H], qkv[:, H:H + Hkv], qkv[:, H + Hkv:]
        att = np.zeros((T, H, D))
        for hq in range(H):
            hk = hq // (H // Hkv)
            sc = np.where(causal, (q[:, hq] @ k[:, hk].T) / np.sqrt(D), -np.inf)
            p = np.exp(sc - sc.max(-1, keepdims=True))
            att[:, hq] = _f16((p @ v[:, hk]) / p.sum(-1, keepdims=True))
        part = lin(f"layers.{l}.attention.wo", att.reshape(T, H * D))
        xn, h = _rms(h, part, g(f"layers.{l}.ffn_norm.weight"), desc.norm_eps)
        gu = _f16(xn @ g(f"layers.{l}.feed_forward.w13.weight").reshape(-1, hd).T)
        inter = gu.shape[1] // 2
        act = _f16(gu[:, :inter] / (1 + np.exp(-gu[:, :inter])) * gu[:, inter:])
        pending = lin(f"layers.{l}.feed_forward.w2", act)
    hn, _ = _rms(h[-1:], pending[-1:], g("norm.weight"), desc.norm_eps)
    return (hn @ g("output.weight").reshape(-1, hd).T)[0]


def extra_rounding_error(geom, prompt_len=33, seed=7):
    """{'model_vs_oracle': how far numpy_forward is from the oracle on the base weights, adapter id: max |logit difference| / max(1,
    |logit|max) between the merged model (one rounding per linear) and the adapter arithmetic of tests/lora.py (y0 rounded, t rounded, the
    sum rounded) -- both with exact sums, so the figure is what the two extra roundings alone are worth}"""
    desc = make_desc(geom, "fp16")
    W = base_weights(desc)
    sh, _ = shapes(desc)
    prompt = np.random.RandomState(seed).randint(3, desc.vocab_size, size=prompt_len)

    def mat(weights, n):
        return weights[n + ".weight"].astype(np.float64).reshape(sh[n.split(".", 2)[2]])

    rm = oracle(desc, W, 64)
    want = ref.forward([rm], ref.make_step(prompt.astype(np.int64), [0, prompt_len], [0], [0], 0))[0]
    rm.close()
    base = numpy_forward(desc, W, prompt, lambda n, x: _f16(x @ mat(W, n).T))
    out = {"model_vs_oracle": float(np.abs(base - want).max() / max(1.0, np.abs(want).max()))}
    for aid in ADAPTERS:
        t, scale = make_adapter(desc, aid)
        Wm = merged(W, t, scale)

        def device(n, x):
            y0 = _f16(x @ mat(W, n).T)
            if n + ".lora_a" not in t:
                return y0
            tt = _f16(x @ t[n + ".lora_a"].astype(np.float64).T)
            return _f16(y0 + scale * (tt @ t[n + ".lora_b"].astype(np.float64).T))

        m_ = numpy_forward(desc, Wm, prompt, lambda n, x: _f16(x @ mat(Wm, n).T))
        d_ = numpy_forward(desc, W, prompt, device)
        out[aid] = float(np.abs(m_ - d_).max() / max(1.0, np.abs(m_).max()))
    return out
