"""The model of the multi-LoRA GPU tests without a device (tests/lora_model.py): every merge is exact, the adapters change the logits by
far more than the bar, and the merged oracles alone give the greedy-token comparison enough rows outside the near-tie margin."""
import numpy as np
import pytest

from tests import lora_model as LM

MIN_SAFE_FRACTION = 0.75      # tests/test_gpu_model.py check_steps


@pytest.mark.parametrize("geom,kv", sorted(LM.K_CAP))
def test_merged_oracles_meet_the_greedy_floor(geom, kv):
    tr = LM.Trace(LM.make_desc(geom, kv))            # (merged() asserts W + scale B A is exactly an fp16 matrix, for every adapter)
    assert sorted(tr.oracles) == [-1, 0, 1, 2]
    safe = {g: [0, 0] for g in tr.oracles}
    moved = {g: 0.0 for g in tr.oracles if g >= 0}
    shapes = []
    for s, args, slots, want, alt in tr.steps():
        shapes.append((len(slots), len(args[0]), int(args[4])))
        scale = max(1.0, float(np.abs(want).max()))
        srt = np.sort(want, -1)
        margin = srt[:, -1] - srt[:, -2]
        base = None
        for g in tr.oracles:
            rows = np.nonzero(slots == g)[0]
            tol = 1e-3 * LM.K_CAP[(geom, kv)][g] * max(1.0, float(np.abs(want[rows]).max()))
            safe[g][0] += int((margin[rows] > 2 * tol).sum())
            safe[g][1] += len(rows)
        if s == 0:
            from oracle import ref
            base = ref.forward([tr.oracles[-1]], ref.make_step(*args))
            for g in moved:
                rows = np.nonzero(slots == g)[0]
                moved[g] = float(np.abs(want[rows] - base[rows]).max() / scale)
    # the issue's run: a packed prefill of eight requests, three decode steps, a mixed step that a ninth request joins
    assert shapes == [(8, sum(LM.PROMPT_LENS), 0), (8, 8, 8), (8, 8, 8), (8, 8, 8), (9, 8 + LM.JOIN_LEN, 8)]
    for g, (n_safe, n_rows) in safe.items():
        assert n_safe >= MIN_SAFE_FRACTION * n_rows, (g, n_safe, n_rows)
    # an adapter's oracle is not the base oracle in disguise: already in the prefill step it moves the logits of its requests by more
    # than four times its group's cap (a device that dropped the adapter would miss the bar by that factor)
    print(geom, kv, "adapters move the prefill logits by", moved)
    assert all(v > 4 * 1e-3 * LM.K_CAP[(geom, kv)][g] for g, v in moved.items()), moved


@pytest.mark.parametrize("geom", ["mha", "gqa"])
def test_the_extra_roundings_alone_are_worth_a_no_adapter_error(geom):
    """Evidence for the caps of the adapter groups (tests/test_gpu_lora_model.py): with EXACT sums everywhere, the adapter arithmetic --
    y0 rounded, t rounded, the sum rounded, on three of the four linears of a layer -- against the merged model's one rounding per linear
    moves the last-token logits of a 33-token prompt by 0.19e-3 .. 0.27e-3 of the logit scale.  The device's rows without an adapter are
    0.18e-3 .. 0.23e-3 from the oracle (summation order), so an adapter row starts from about twice that; the int8-g8 KV of the
    grouped-query case (a quantiser turns a one-ulp difference into a cache LSB) is not in this model."""
    r = LM.extra_rounding_error(geom)
    print(geom, r)
    assert r["model_vs_oracle"] < 1e-4, "the numpy model is not the specification"
    for aid in LM.ADAPTERS:
        assert 0.1e-3 < r[aid] < 0.5e-3, (aid, r[aid])
