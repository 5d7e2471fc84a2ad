"""ALiBi attention inside the step (pplhip_alibi): a one-layer fp16-weight, fp16-KV, head_dim-128 context against a float64 numpy
restatement of that layer without rotation -- embedding, RMSNorm, wqkv, ALiBi attention, wo, SwiGLU, final norm, lm_head -- over a prefill of
two prompts and three greedy decode steps.  Cap: 1.5e-3 x max(1, max |logit|), the one tests/test_gpu_model.py applies to its shallow fp16
fixture (check_steps(k=1.5) for ("mha", 0), line 135).  The same context without pplhip_alibi must lie outside it."""
import numpy as np
import pytest

from oracle import ref
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HID, INTER, H, D, VOCAB, EPS = 256, 512, 2, 128, 1024, 1e-5
SLOPES = [0.5, 2.0 ** -4]
CAP = 1.5e-3


def make_ctx(m, **kw):
    args = dict(hidden_dim=HID, intermediate_dim=INTER, num_layers=1, num_heads=H, num_kv_heads=H, vocab_size=VOCAB, max_position=512,
                norm_eps=EPS, cache_layout=3, cache_mode=1, page_size=16)
    args.update(kw)
    ctx = m.Context(m.copy_desc(ref.make_desc(**args)), max_running_batch=8, max_tokens_per_step=256)
    return ctx


def weights():
    rng = np.random.RandomState(11)
    w = {"tok_embeddings.weight": rng.randn(VOCAB, HID), "norm.weight": 1 + 0.1 * rng.randn(HID), "output.weight": rng.randn(VOCAB, HID) / 16,
         "layers.0.attention_norm.weight": 1 + 0.1 * rng.randn(HID), "layers.0.ffn_norm.weight": 1 + 0.1 * rng.randn(HID),
         "layers.0.attention.wqkv.weight": rng.randn(3 * H * D, HID) / 8, "layers.0.attention.wo.weight": rng.randn(HID, H * D) / 16,
         "layers.0.feed_forward.w13.weight": rng.randn(2 * INTER, HID) / 16, "layers.0.feed_forward.w2.weight": rng.randn(HID, INTER) / 16}
    return {k: v.astype(np.float16) for k, v in w.items()}


def numpy_trace(w, prompts, steps, slopes):
    """float64 logits of the prefill and of `steps` greedy decode steps; the tokens it chose drive the device too"""
    w = {k: v.astype(np.float64) for k, v in w.items()}
    norm = lambda x, g: x / np.sqrt((x * x).mean(-1, keepdims=True) + EPS) * g
    keys, vals, out, toks = [[] for _ in prompts], [[] for _ in prompts], [], []
    new = [list(p) for p in prompts]
    for _ in range(steps + 1):
        logits = []
        for b, tk in enumerate(new):
            x = w["tok_embeddings.weight"][tk]
            qkv = (norm(x, w["layers.0.attention_norm.weight"]) @ w["layers.0.attention.wqkv.weight"].T).reshape(len(tk), 3 * H, D)
            att = np.empty((len(tk), H, D))
            for i in range(len(tk)):
                keys[b].append(qkv[i, H:2 * H]); vals[b].append(qkv[i, 2 * H:])
                K, V, p = np.array(keys[b]), np.array(vals[b]), len(keys[b]) - 1
                for h in range(H):
                    s = K[:, h] @ qkv[i, h] / np.sqrt(D) + slopes[h] * (np.arange(p + 1) - p)
                    e = np.exp(s - s.max())
                    att[i, h] = (e / e.sum()) @ V[:, h]
            x = x + att.reshape(len(tk), -1) @ w["layers.0.attention.wo.weight"].T
            gu = norm(x, w["layers.0.ffn_norm.weight"]) @ w["layers.0.feed_forward.w13.weight"].T
            g, u = gu[:, :INTER], gu[:, INTER:]
            x = x + (g / (1 + np.exp(-g)) * u) @ w["layers.0.feed_forward.w2.weight"].T
            logits.append(norm(x[-1], w["norm.weight"]) @ w["output.weight"].T)
        out.append(np.array(logits))
        toks.append(out[-1].argmax(axis=1))
        new = [[t] for t in toks[-1]]
    return out, toks


def device_trace(m, w, prompts, toks, alibi):
    ctx = make_ctx(m)
    if alibi is not None:
        ctx.alibi(alibi)
    for k, v in w.items():
        ctx.set_tensor(0, k, v)
    ctx.kv_alloc(0, 1024)
    B = len(prompts)
    pages = (np.arange(B * 8, dtype=np.int64).reshape(B, 8) * 7) % (B * 8)   # every request 8 pages of its own, out of order
    lens = np.array([len(p) for p in prompts])
    tok, seq, sp, out = np.concatenate(prompts).astype(np.int64), np.concatenate([[0], np.cumsum(lens)]), np.zeros(B, dtype=np.int64), []
    for s in range(len(toks)):
        ctx.set_inputs(0, m.make_step(tok, seq, sp, pages, 0 if s == 0 else B, 8, req_list_changed=int(s < 2)))
        ctx.run(0, cache_prefill=0)
        out.append(ctx.copy_logits(B).copy())
        tok, sp, seq = toks[s].astype(np.int64), sp + (seq[1:] - seq[:-1]), np.arange(B + 1)
    ctx.close()
    return out


def distance(got, want):
    return max(float(np.abs(g - x).max() / max(1.0, np.abs(x).max())) for g, x in zip(got, want))


def test_alibi_context_matches_the_float64_layer_and_a_rotary_context_does_not():
    m, rng, w = load_pplhip(), np.random.RandomState(3), weights()
    prompts = [rng.randint(3, VOCAB, size=n) for n in (70, 48)]
    want, toks = numpy_trace(w, prompts, 3, SLOPES)
    d_alibi, d_plain = distance(device_trace(m, w, prompts, toks, SLOPES), want), distance(device_trace(m, w, prompts, toks, None), want)
    print(f"distance to the float64 ALiBi layer / max |logit|: under pplhip_alibi {d_alibi:.3e} (cap {CAP:.1e}), rotary context {d_plain:.3e}")
    assert d_alibi <= CAP
    assert d_plain > CAP   # a path that ignored the slopes (and rotated) could not pass


def test_context_without_alibi_is_untouched():
    """a context that never calls pplhip_alibi against a second one: the same bits on one step"""
    m, rng, w = load_pplhip(), np.random.RandomState(4), weights()
    prompts = [rng.randint(3, VOCAB, size=n) for n in (20, 9)]
    toks = [np.array([5, 6])]
    a, b = device_trace(m, w, prompts, toks, None), device_trace(m, w, prompts, toks, None)
    assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all()


@pytest.mark.parametrize("other", ["sliding_window", "shared_prefix"])
def test_alibi_refuses_window_and_shared_prefix_in_both_orders(other):
    m = load_pplhip()
    on = {"sliding_window": lambda c: m.lib().pplhip_sliding_window(c.h, 24), "shared_prefix": lambda c: m.lib().pplhip_shared_prefix(c.h, 2, 16)}[other]
    ctx = make_ctx(m)
    assert on(ctx) == 0 and m.lib().pplhip_alibi(ctx.h, None) == -7
    ctx.close()
    ctx = make_ctx(m)
    ctx.alibi()
    assert on(ctx) == -7
    ctx.close()
