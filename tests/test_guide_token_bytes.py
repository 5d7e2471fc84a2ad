"""Tokenizer::TokenBytes of the SentencePiece tokenizers (through build/guide_trace vocab), the bytes guided decoding walks: a NORMAL or
USER_DEFINED piece is its bytes with U+2581 as a space, a BYTE piece its one byte, CONTROL / UNKNOWN / UNUSED pieces and ids at or behind
the piece count are empty, and nothing is stripped."""
import pytest

from tests import guide as G
from tests.conftest import ROOT

MODELS = ["spm_bpe.model", "spm_unigram.model", "spm_unigram_nofb.model"]


@pytest.mark.parametrize("model", MODELS)
def test_against_the_sentencepiece_module(model):
    spm = pytest.importorskip("sentencepiece")
    sp = spm.SentencePieceProcessor(model_file=f"{ROOT}/tests/golden/{model}")
    toks, n, eos = G.spm_vocab(model)
    assert n == sp.get_piece_size() and eos == sp.eos_id() and len(toks) == n + 2
    for i in range(n):
        piece = sp.id_to_piece(i)
        if sp.is_byte(i):
            want = bytes([int(piece[3:5], 16)])
        elif sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i):
            want = b""
        else:
            want = piece.replace("▁", " ").encode("utf-8")
        assert toks[i] == want, (i, piece)
    assert toks[n] == toks[n + 1] == b""


def test_properties_without_the_module():
    toks, n, eos = G.spm_vocab("spm_bpe.model")
    assert n == 420 and toks[eos] == b"" and toks[n] == toks[n + 1] == b""
    assert {t for t in toks if len(t) == 1} == {bytes([b]) for b in range(256)}      # byte fallback: every byte has a piece
    assert not any(b"\xe2\x96\x81" in t for t in toks)                                 # U+2581 became a space
    assert any(t.startswith(b" ") and len(t) > 1 for t in toks)                        # and the space in front of a word is kept
    nofb, n2, _ = G.spm_vocab("spm_unigram_nofb.model")
    assert not any(t[:1] in (b"7", b"9", b"Q", b"{") for t in nofb)                    # what tests/test_gpu_guide_model.py counts on
