"""Long prompts on the host (no GPU): the 75-token window split of encode_tokens against the golden vectors written by the
reference's own encode_tokens (tools/gen_golden_encode_tokens.py), the oracle text encoder per window against the same vectors,
and the tokenizer calls of PromptEncoder with and without max_length."""
import numpy as np
import pytest
import torch

from tests.long_prompt_util import BOS, EOS, FakeTokenizer, expected_windows
from tests.util import load_npz

WIDTHS = (60, 77, 78, 100, 152, 225)


@pytest.fixture(scope="module")
def golden():
    return load_npz("encode_tokens_tiny.npz")


def test_golden_covers_the_issue_widths(golden):
    assert tuple(int(w) for w in golden["widths"]) == WIDTHS
    for w in WIDTHS:
        ids, hid = golden[f"ids_{w}"], golden[f"hidden_{w}"]
        assert ids.shape == (2, w) and hid.dtype == np.float32
        assert (ids[0] == EOS).sum() < (ids[1] == EOS).sum()          # rows of different true length, padded with the pad id


@pytest.mark.parametrize("w", WIDTHS)
def test_window_split_matches_golden_lengths(golden, w):
    from sketch2img_amd.clip_text import split_windows
    ids = torch.from_numpy(golden[f"ids_{w}"])
    wins = split_windows(ids, BOS, EOS)
    nwin = 0 if w <= 77 else -(-w // 75)
    assert [x.shape[1] for x in wins] == expected_windows(w) and len(wins) == max(1, nwin)
    assert sum(x.shape[1] for x in wins) == w + 2 * nwin == golden[f"hidden_{w}"].shape[1]
    if nwin == 0:
        assert wins[0] is ids or torch.equal(wins[0], ids)
        return
    # raw ids: the prompt's own BOS / EOS and the collate padding stay inside the windows, in order
    assert torch.equal(torch.cat([x[:, 1:-1] for x in wins], 1), ids)
    for x in wins:
        assert bool((x[:, 0] == BOS).all()) and bool((x[:, -1] == EOS).all())


@pytest.mark.parametrize("w", WIDTHS)
def test_oracle_per_window_matches_golden(golden, w):
    """oracle.clip_text.last_hidden_state per window, concatenated, against the reference's encode_tokens on transformers'
    CLIPTextModel: the bound test_oracle.py uses for clip_text_tiny.npz (5e-6 absolute)."""
    from oracle import clip_text as ot
    from sketch2img_amd.clip_text import split_windows
    W = ot.init_weights(ot.TINY_TEXT)
    wins = split_windows(torch.from_numpy(golden[f"ids_{w}"]), BOS, EOS)
    out = torch.cat([ot.last_hidden_state(ot.TINY_TEXT, W, x) for x in wins], 1)
    ref = torch.from_numpy(golden[f"hidden_{w}"])
    assert out.shape == ref.shape
    err = float((out - ref).abs().max())
    print(f"[parity] oracle windows width {w}: max={err:.3e}")
    assert err < 5e-6


class _RecordingModel:
    """Stands in for the CLIPTextModel facade: records the id matrices, returns zeros of the right shape."""

    def __init__(self):
        from sketch2img_amd.config import TINY_TEXT
        self.cfg, self.seen = TINY_TEXT, []

    def __call__(self, ids):
        self.seen.append(ids.clone())
        return (torch.zeros(ids.shape[0], ids.shape[1], self.cfg.hidden_size, dtype=torch.float16),)


def test_prompt_encoder_default_path_calls_tokenizer_as_before():
    from sketch2img_amd.clip_text import PromptEncoder
    tok, model = FakeTokenizer(), _RecordingModel()
    enc = PromptEncoder(tok, model)
    assert enc.max_length is None
    out = enc(["a cat", " ".join(["tag"] * 120)])
    assert tok.calls == [("call", ["a cat", " ".join(["tag"] * 120)],
                          dict(padding="max_length", max_length=77, truncation=True, return_tensors="pt"))]
    assert len(model.seen) == 1 and model.seen[0].shape == (2, 77) and out.shape == (2, 77, 64)


def test_prompt_encoder_max_length_widths():
    from sketch2img_amd.clip_text import PromptEncoder
    tok, model = FakeTokenizer(), _RecordingModel()
    enc = PromptEncoder(tok, model, max_length=225)
    long = " ".join(f"w{i}" for i in range(120))              # 120 words + BOS + EOS = 122 ids
    ids = enc.tokenize([long])
    assert ids.shape == (1, 122)
    assert tok.calls[0] == ("call", [long], dict(padding="do_not_pad", truncation=True, max_length=225))
    assert tok.calls[1] == ("pad", None, dict(padding=True, return_tensors="pt"))
    out = enc([long])
    assert out.shape == (1, 122 + 2 * 2, 64)                  # windows of 75 and 47 ids, each in BOS / EOS
    assert model.seen[-1].shape == (2, 77)                    # one pass: both windows as rows of 77
    assert torch.equal(model.seen[-1][0, 1:76], ids[0, :75]) and torch.equal(model.seen[-1][1, 1:48], ids[0, 75:])
    # truncation at max_length, and a short prompt stays at its own length
    assert enc.tokenize([" ".join(["x"] * 400)]).shape == (1, 225) and enc([" ".join(["x"] * 400)]).shape == (1, 231, 64)
    assert enc(["a cat"]).shape == (1, 4, 64)
    with pytest.raises(ValueError):
        PromptEncoder(tok, model, max_length=0)


def test_negatives_and_prompts_share_one_width():
    """_encode_prompt with a max_length encoder: one call for [negatives; prompts], so both CFG halves have the same key count."""
    from sketch2img_amd.clip_text import PromptEncoder
    from sketch2img_amd.modules.pipeline import AntiGradientPipeline
    tok, model = FakeTokenizer(), _RecordingModel()
    pipe = AntiGradientPipeline.__new__(AntiGradientPipeline)
    pipe.text_encoder, pipe.allow_pseudo_text = PromptEncoder(tok, model, max_length=225), False
    long = " ".join(f"w{i}" for i in range(120))
    ehs = pipe._encode_prompt([long, "a dog"], "cpu", 2, True, None)
    assert ehs.shape == (8, 126, 64)                          # [2 negatives x 2; 2 prompts x 2], all at the long prompt's width
    assert [c[0] for c in tok.calls] == ["call", "pad"] and tok.calls[0][1] == ["", "", long, "a dog"]
    # today's encoder (no max_length): two calls, as before
    tok2 = FakeTokenizer()
    pipe.text_encoder = PromptEncoder(tok2, model)
    assert pipe._encode_prompt("a dog", "cpu", 1, True, "bad").shape == (2, 77, 64)
    assert [c[1] for c in tok2.calls] == [["a dog"], ["bad"]]


def test_encode_tokens_is_reexported_by_sat_train():
    from sketch2img_amd import clip_text, sat_train
    assert sat_train.encode_tokens is clip_text.encode_tokens
