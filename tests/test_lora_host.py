"""Per-request LoRA adapters on the host side (tests/host/lora_trace.cc: the generator and the engine over a fake backend and the adapter
registry): the prefix cache never shares pages across adapters or across loads of a slot, a slot that a request names cannot be unloaded,
and the packed adapter slots follow the batch rows."""
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "lora_trace")


@pytest.fixture(scope="module")
def trace():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _first_step(trace, phase):
    return next(r for r in trace if r.get("phase") == phase and r["step"] == 0)


def _events(trace, name):
    return [r for r in trace if r.get("event") == name]


def test_prefix_cache_is_keyed_by_the_adapter(trace):
    assert _events(trace, "loaded")[0]["uids_differ"] == 1
    no_hit = dict(prefix_hit=0, start_pos=[0], num_tokens=13)
    hit = dict(prefix_hit=1, start_pos=[12], num_tokens=1)       # three cached pages of four tokens, the 13th token is fed
    for phase, want in [("base_first", no_hit),
                        ("adapter0_first", no_hit),              # same tokens, different adapters: no hit
                        ("adapter0_again", hit),                 # same adapter: hit
                        ("adapter1_first", no_hit),
                        ("base_again", hit),                     # without an adapter nothing changed
                        ("adapter0_reloaded", no_hit),           # reloaded slot: a new uid, no hit
                        ("adapter1_running", hit)]:
        r = _first_step(trace, phase)
        assert {k: r[k] for k in want} == want, (phase, r)
    assert _events(trace, "reloaded")[0]["uid_is_new"] == 1


def test_a_slot_that_a_request_names_is_not_unloaded(trace):
    assert _events(trace, "unload_idle")[0]["rc"] == 1
    assert _events(trace, "unload_while_running") == [{"event": "unload_while_running", "slot": 1, "rc": 0}]     # refused
    # the request ran to its end on the adapter
    steps = [r for r in trace if r.get("phase") == "adapter1_running"]
    assert len(steps) == 6 and all(r["lora_slots"] == [1] for r in steps)
    assert _events(trace, "unload_after")[0]["rc"] == 1 and _events(trace, "unload_twice")[0]["rc"] == -1
    failed = {r["failed"]: r for r in trace if "failed" in r}
    assert set(failed) == {8, 9} and all(r["rc"] == 2 and "not loaded" in r["msg"] for r in failed.values())
    assert [r["rc"] for r in _events(trace, "unload_end")] == [1, 1]      # every request gave its reference back


def test_packed_slots_follow_the_batch_rows(trace):
    steps = [r for r in trace if r.get("phase") == "batch_order"]
    backend = [r for r in trace if "backend" in r][-len(steps):]
    assert len(steps) >= 8
    seen = set()
    sizes = []
    for st, be in zip(steps, backend):
        ids = [t - 500 for t in be["last_tokens"]]                # the fake model repeats the prompt's last token, 500 + id
        want = [i % 3 - 1 for i in ids]
        assert st["lora_slots"] == want, (st, be)
        if any(s >= 0 for s in want):
            assert be["has_slots"] == 1 and be["lora_slots"] == want
        else:
            assert be["has_slots"] == 0                           # a step without adapters is handed no slots at all
        seen |= set(ids)
        sizes.append(len(ids))
    assert seen == {1, 2, 3, 4, 5, 6}
    assert max(sizes) == 4 and any(a > b for a, b in zip(sizes, sizes[1:])), "rows were freed and refilled"
    # rows were reused: request 5 entered after request 1 left
    first5 = next(i for i, be in enumerate(backend) if 505 in be["last_tokens"])
    assert all(501 not in be["last_tokens"] for be in backend[first5:])
    # steps of the phases without any adapter hand the backend none either
    base = [r for r in trace if "backend" in r][:2]
    assert all(b["has_slots"] == 0 for b in base)
