"""JSON-schema guides through the whole host stack on the GPU: a scenario through tools/offline_inference in which one request carries
guide_json_schema (as an object, which the reader writes out again, and as a string), one carries guide_regex and the others nothing; the
same through pplsrv_submit_guided_json of the serving C API; and --guide-json-schema FILE for the other workloads.  The schemas have finite
languages whose longest document, at one byte per token, fits generation_length, so every guided answer ends on the end token: it must
parse as JSON and fit its schema.  The regex and the plain requests answer exactly as they do in a run without the schema's requests."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import pytest

from tests import guide as G8
from tests import guide16 as G
from tests.conftest import ROOT
from tests.test_gpu_tools import CFG, PKG

pytestmark = pytest.mark.gpu
SPM = os.path.join(ROOT, "tests", "golden", "spm_bpe.model")
COLOURS = ["red", "green", "blue", "é\"\\"]
SCHEMA = {"type": "object", "properties": {"colour": {"enum": COLOURS}, "sizes": {"type": "array", "items": {"enum": [1, 2, 3]}, "maxItems": 3},
                                            "note": {"type": "string", "maxLength": 4}, "ok": {"type": "boolean"}},
          "required": ["colour", "sizes"]}
LIST = {"type": "array", "items": {"type": ["boolean", "null"]}, "minItems": 1, "maxItems": 4}
REGEX = "[0-9]{3}-[0-9]{4}"
GEN = 120


def fits(doc, schema):
    if schema is LIST:
        return isinstance(doc, list) and 1 <= len(doc) <= 4 and all(x is None or isinstance(x, bool) for x in doc)
    keys = [k for k in ("colour", "sizes", "note", "ok") if k in doc]
    return (isinstance(doc, dict) and list(doc) == keys and doc.get("colour") in COLOURS and isinstance(doc.get("sizes"), list)
            and len(doc["sizes"]) <= 3 and all(x in (1, 2, 3) and not isinstance(x, bool) for x in doc["sizes"])
            and isinstance(doc.get("note", ""), str) and len(doc.get("note", "")) <= 4 and isinstance(doc.get("ok", True), bool))


def test_the_longest_documents_fit_the_generation_length():
    """on the CPU: the languages are finite, and their longest documents, at one byte per token and with the end token, fit GEN"""
    for schema in (SCHEMA, LIST):
        n = G.longest(*G.compile_schema(schema))
        assert n is not None and n + 1 <= GEN, n


def _offline(args):
    tool = os.path.join(PKG, "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    cmd = [tool, "--model-param-path", CFG, "--synthetic-weights", "--tokenizer-path", SPM] + args
    return subprocess.check_output(cmd, timeout=300, stderr=subprocess.DEVNULL).decode()


def _scenario(path, reqs):
    json.dump({"generator": {"max_running_batch": 8, "max_tokens_per_step": 64, "max_prefill_batch": 8, "enable_penalty": False},
               "kv_cache_max_tokens": 2048, "requests": reqs}, open(path, "w"), ensure_ascii=False)
    return json.loads(_offline(["--workload", "scenario", "--scenario-file", path]).strip().splitlines()[-1])


def test_scenario_through_offline_inference(tmp_path):
    pieces, n, eos = G8.spm_vocab()
    reqs = [dict(id=i, tokens=[10 * i + 11 + j for j in range(2 + i)], top_k=1, generation_length=GEN, early_stopping=True) for i in range(7)]
    reqs[0]["guide_json_schema"] = SCHEMA                              # an object: the reader writes it out again, keys in their order
    reqs[2]["guide_regex"] = REGEX
    reqs[3]["guide_json_schema"] = json.dumps(LIST)                    # a string
    reqs[5]["guide_json_schema"] = {"type": "string", "pattern": "a+"}  # outside the subset: this request fails, alone
    reqs[6]["guide_json_schema"] = SCHEMA
    reqs[6]["guide_regex"] = REGEX                                     # both: fails alone
    for r in (reqs[1], reqs[4]):
        r["generation_length"] = 12
    path = str(tmp_path / "scenario.json")
    res = _scenario(path, reqs)
    assert res["failed"] == [5, 6] and sorted(res["tokens"]) == ["0", "1", "2", "3", "4"]
    for i, schema in ((0, SCHEMA), (3, LIST)):
        toks = res["tokens"][str(i)]
        assert toks[-1] == eos and len(toks) <= GEN, (i, toks)        # it ended on the end token
        text = b"".join(pieces[t] for t in toks[:-1])
        assert fits(json.loads(text.decode("utf-8")), schema), text
    text = b"".join(pieces[t] for t in res["tokens"]["2"][:-1])
    assert re.fullmatch(REGEX.encode(), text), text
    # the regex and the plain requests answer as they do without the schemas' requests
    alone = _scenario(path, [r for r in reqs if "guide_json_schema" not in r])
    assert alone["failed"] == []
    for i in (1, 2, 4):
        assert res["tokens"][str(i)] == alone["tokens"][str(i)], i


def test_guide_json_schema_flag(tmp_path):
    """--guide-json-schema FILE gives every request of prompts4 the schema: a boolean fits the shortest generation length (8 tokens)"""
    pieces, n, eos = G8.spm_vocab()
    assert G.longest(*G.compile_schema({"type": "boolean"})) + 1 <= 8
    path = str(tmp_path / "schema.json")
    json.dump({"type": "boolean"}, open(path, "w"))
    out = _offline(["--workload", "prompts4", "--guide-json-schema", path, "--max-running-batch", "8", "--max-tokens-per-step", "64",
                    "--kv-cache-max-tokens", "2048"])      # (small buffers: the defaults take seconds to set up)
    answers = [line.split()[2:] for line in out.splitlines() if line.startswith("Answer tokens:")]
    assert len(answers) == 4
    for toks in answers:
        toks = [int(t) for t in toks]
        assert toks[-1] == eos and json.loads(b"".join(pieces[t] for t in toks[:-1]).decode()) in (True, False), toks


def test_guided_json_through_the_serving_c_api():
    """pplsrv_submit_guided_json, the entry point under the gRPC front end: a schema, a regex and plain requests in one call"""
    pytest.importorskip("grpc")
    sys.path.insert(0, os.path.join(PKG, "serving"))
    import argparse
    import grpc_server as gs
    pieces, n, eos = G8.spm_vocab()
    ap = argparse.ArgumentParser()
    gs.add_flags(ap)
    a = ap.parse_args(["--model-param-path", CFG, "--synthetic-weights", "--synthetic-seed", "77", "--kv-cache-max-tokens", "4096",
                       "--max-running-batch", "16", "--max-tokens-per-step", "256", "--tokenizer-path", SPM])
    lib = gs.load_lib()
    assert hasattr(lib, "pplsrv_submit_guided_json")
    lib.pplsrv_submit_guided_json.argtypes = [C.c_void_p, C.POINTER(gs.CRequest), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                              C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32]
    h = C.c_void_p()
    assert lib.pplsrv_create_ex(C.byref(gs.make_config(a)), 0, 0, C.byref(h)) == 0
    next_id = [0]

    def ask(guides):
        """guides: per request None, ("regex", text) or ("schema", text)"""
        cnt = len(guides)
        keep, reqs, rx, js = [], (gs.CRequest * cnt)(), (C.c_char_p * cnt)(), (C.c_char_p * cnt)()
        base = next_id[0]
        next_id[0] += cnt
        for i, g in enumerate(guides):
            toks = (C.c_int32 * 3)(5, 6, 7 + i)
            keep.append(toks)
            q = reqs[i]
            q.id, q.tokens, q.n_tokens = base + i, toks, 3
            q.temperature, q.top_p, q.top_k, q.repetition_penalty, q.generation_length, q.early_stopping = 1.0, 0.0, 1, 1.0, GEN if g else 10, 1
            rx[i] = g[1].encode() if g and g[0] in ("regex", "both") else None
            js[i] = (g[2] if g[0] == "both" else g[1]).encode() if g and g[0] in ("schema", "both") else (b"" if i % 2 else None)
        assert lib.pplsrv_submit_guided_json(h, reqs, None, None, None, None, None, rx, js, cnt) == 0
        seen, failed, done = {base + i: [] for i in range(cnt)}, [], 0
        buf = (gs.CResponse * 64)()
        t0 = time.time()
        while done < cnt and time.time() - t0 < 120:
            for k in range(lib.pplsrv_poll(h, buf, 64, 50)):
                r = buf[k]
                if r.status == gs.P.FAILED:
                    failed.append(r.id - base)
                else:
                    seen[r.id].append(r.token)
                done += r.status != gs.P.PROCESSING
        assert done == cnt
        return [seen[base + i] for i in range(cnt)], failed

    try:
        base, failed = ask([None, None, ("regex", REGEX), None, None, None])
        assert failed == []
        seen, failed = ask([("schema", json.dumps(SCHEMA, ensure_ascii=False)), None, ("regex", REGEX), None,
                            ("schema", '{"type": "integer", "minimum": 0}'), ("both", REGEX, json.dumps(LIST))])
        assert sorted(failed) == [4, 5] and seen[4] == [] and seen[5] == []
        assert seen[0][-1] == eos
        assert fits(json.loads(b"".join(pieces[t] for t in seen[0][:-1]).decode("utf-8")), SCHEMA)
        assert re.fullmatch(REGEX.encode(), b"".join(pieces[t] for t in seen[2][:-1]))
        for i in (1, 2, 3):                              # the regex and the plain neighbours answer as before
            assert seen[i] == base[i], i
    finally:
        lib.pplsrv_destroy(h)
