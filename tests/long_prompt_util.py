"""Helpers shared by tests/test_host_long_prompts.py and tests/test_gpu_long_prompts.py: a word-level stand-in for CLIPTokenizer
with transformers' call convention (records every call), and the expected window arithmetic of encode_tokens."""
import torch

BOS, EOS = 998, 999          # TINY_TEXT: vocab_size - 2 / - 1, as the golden generators use them


def expected_windows(width):
    """Widths of the id matrices encode_tokens encodes for an id matrix of `width` columns (modules/clip_guided_trainer.py:40-66)."""
    if width <= 77:
        return [width]
    return [min(75, width - c) + 2 for c in range(0, width, 75)]


class FakeTokenizer:
    """One id per whitespace-separated word (stable in the word), BOS in front, EOS behind, EOS as the pad id."""
    bos_token_id, eos_token_id, pad_token_id, model_max_length = BOS, EOS, EOS, 77

    def __init__(self):
        self.calls = []

    @staticmethod
    def _word(w):
        return sum((i + 1) * ord(c) for i, c in enumerate(w)) % 990 + 1

    def __call__(self, prompts, **kw):
        self.calls.append(("call", list(prompts), dict(kw)))
        rows = [[BOS] + [self._word(w) for w in p.split()] + [EOS] for p in prompts]
        if kw.get("truncation"):
            rows = [r if len(r) <= kw["max_length"] else r[:kw["max_length"] - 1] + [EOS] for r in rows]
        if kw.get("padding") == "max_length":
            rows = [r + [EOS] * (kw["max_length"] - len(r)) for r in rows]
        if kw.get("return_tensors") == "pt":
            return {"input_ids": torch.tensor(rows, dtype=torch.long)}
        return {"input_ids": rows}

    def pad(self, enc, **kw):
        self.calls.append(("pad", None, dict(kw)))
        rows = enc["input_ids"]
        W = max(len(r) for r in rows)
        return {"input_ids": torch.tensor([list(r) + [EOS] * (W - len(r)) for r in rows], dtype=torch.long)}
