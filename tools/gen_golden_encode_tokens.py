#!/usr/bin/env python3
"""Golden vectors of the long-prompt encoding (checked by tests/test_host_long_prompts.py and tests/test_gpu_long_prompts.py):
the reference's OWN ``encode_tokens`` (modules/clip_guided_trainer.py:40-66) on transformers' CLIPTextModel at TINY_TEXT with the
seeded weights of tools/gen_golden_clip_text.py.  Runs in the build container only: needs `transformers` and the reference tree
(``--reference DIR`` or $SKETCH2IMG_REFERENCE).  That one function is loaded from the tree at run time - the module's other
imports (bitsandbytes, accelerate, torchtext, ...) are replaced by empty stub modules - and nothing of its text is kept.

Writes tests/golden/encode_tokens_tiny.npz = {widths, ids_<W> int64 [2, W], hidden_<W> fp32 [2, L, 64]} for the id-matrix widths
60, 77 (encoded as they are), 78, 100, 152 and 225 (75-token windows: L = W + 2 * ceil(W / 75) = 82, 104, 158, 231).  Rows have
different true lengths and are padded with the pad id, as the reference's collate_fn leaves them."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch
from transformers import CLIPTextConfig, CLIPTextModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sketch2img_amd import synthetic  # noqa: E402  (seeded weight recipe only; no arithmetic of ours enters the vector)
from sketch2img_amd.config import TINY_TEXT  # noqa: E402

WIDTHS = (60, 77, 78, 100, 152, 225)


def load_reference_encode_tokens(ref_root: str):
    """``encode_tokens`` out of <ref_root>/modules/clip_guided_trainer.py.  Every import of that file resolves to a stub module
    (attribute access yields further stubs), except torch, which the function needs."""
    path = os.path.join(ref_root, "modules", "clip_guided_trainer.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)

    class Stub(types.ModuleType):
        __path__ = []

        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return Stub(self.__name__ + "." + name)

    keep = {"torch", "math", "os", "itertools", "contextlib", "argparse", "tempfile"}
    added = []
    for node in ast.walk(tree):
        names = []
        if isinstance(node, ast.Import):
            names = [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom) and node.module:
            names = [node.module]
        for n in names:
            parts = n.split(".")
            if parts[0] in keep:
                continue
            for i in range(1, len(parts) + 1):
                key = ".".join(parts[:i])
                if key not in sys.modules:
                    sys.modules[key] = Stub(key)
                    added.append(key)
    # (modules that are already imported - torch, transformers - stay the real ones)
    ns = {"__name__": "reference_clip_guided_trainer"}
    try:
        exec(compile(tree, path, "exec"), ns)
    finally:
        for key in added:
            sys.modules.pop(key, None)
    return ns["encode_tokens"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SKETCH2IMG_REFERENCE"), help="root of the reference tree")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference DIR (or $SKETCH2IMG_REFERENCE) is required")
    encode_tokens = load_reference_encode_tokens(args.reference)

    torch.set_num_threads(1)
    cfg = TINY_TEXT
    bos, eos = cfg.vocab_size - 2, cfg.vocab_size - 1          # as gen_golden_clip_text.py; SD's tokenizer pads with eos
    hf = CLIPTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                        max_position_embeddings=cfg.max_position_embeddings, layer_norm_eps=cfg.layer_norm_eps,
                        hidden_act=cfg.hidden_act, attention_dropout=0.0, bos_token_id=bos, eos_token_id=eos, pad_token_id=eos)
    model = CLIPTextModel(hf).eval()
    W = synthetic.clip_text_state_dict(cfg)
    sd = model.state_dict()
    prefix = "text_model." if any(k.startswith("text_model.") for k in sd) else ""
    missing = model.load_state_dict({prefix + k: v for k, v in W.items()}, strict=False)
    assert not missing.unexpected_keys, missing
    assert all("position_ids" in k for k in missing.missing_keys), missing
    if not hasattr(model, "text_model"):      # transformers >= 5 keeps the transformer's parts on the model itself
        model.__dict__["text_model"] = types.SimpleNamespace(final_layer_norm=model.final_layer_norm)
    tokenizer = types.SimpleNamespace(bos_token_id=bos, eos_token_id=eos)

    g = torch.Generator().manual_seed(11)
    out = {"widths": np.asarray(WIDTHS, dtype=np.int64)}
    for Wd in WIDTHS:
        ids = torch.randint(0, cfg.vocab_size - 2, (2, Wd), generator=g)
        ids[:, 0] = bos
        ids[0, Wd - 1] = eos                                   # row 0 fills the width: [bos, ..., eos]
        n1 = max(3, (2 * Wd) // 3)                             # row 1 is shorter: eos, then the pad id up to the width
        ids[1, n1 - 1:] = eos
        with torch.no_grad():
            h = encode_tokens(tokenizer, model, ids)
        nwin = 0 if Wd <= 77 else -(-Wd // 75)
        assert h.shape == (2, Wd + 2 * nwin, cfg.hidden_size), (Wd, h.shape)
        out[f"ids_{Wd}"] = ids.numpy()
        out[f"hidden_{Wd}"] = h.float().numpy()
        print("transformers", __import__("transformers").__version__, "width", Wd, "->", tuple(h.shape))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "encode_tokens_tiny.npz"), **out)


if __name__ == "__main__":
    main()
