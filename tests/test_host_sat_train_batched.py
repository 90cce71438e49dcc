"""CPU tests (-m "not gpu") of the batched SatMixin training step's host side: the refusals that come before any device work, the
training injector's B-sample begin() / check_rows(), HipUNet.forward's diff_from argument checks."""
from types import SimpleNamespace

import pytest
import torch

from oracle import attn_inject as oinj, unet as ounet
from sketch2img_amd import sat_train
from sketch2img_amd.config import TINY
from sketch2img_amd.unet import HipUNet


def _trainer():
    return sat_train.HipSatTrainer(TINY, oinj.init_state_dict(ounet.TINY, "clip"), "cpu")


def _args(B, h, w):
    z = torch.zeros(B, 4, h, w)
    return z, z, list(range(1, B + 1)), torch.zeros(B, 77, 64), torch.zeros(B, 257, 1024), torch.ones(1000)


@pytest.mark.parametrize("B", [1, 3])
def test_batched_refuses_the_accuracy_mode_before_device_work(B):
    """A net that has nothing but the flag: anything past the refusal would raise AttributeError instead."""
    tr, net = _trainer(), SimpleNamespace(residual_fp32=True)
    with pytest.raises(NotImplementedError, match="accuracy mode"):
        tr.loss_and_grads(net, *_args(B, 16, 16), batched=True)
    with pytest.raises(NotImplementedError, match="accuracy mode"):
        tr.forward_batch(net, *_args(B, 16, 16), batched=True)
    with pytest.raises(NotImplementedError, match="accuracy mode"):
        sat_train.train_step(tr, net, *[_args(B, 16, 16)[i] for i in (0, 3, 4, 2, 1, 5)], batched=True)


def test_batched_refuses_a_non_square_latent_before_device_work():
    tr, net = _trainer(), SimpleNamespace(residual_fp32=False)
    with pytest.raises(AssertionError, match="square maps only"):
        tr.loss_and_grads(net, *_args(2, 16, 24), batched=True)


def test_batched_keyword_is_on_every_entry_point():
    import inspect
    for fn in (sat_train.HipSatTrainer.forward_batch, sat_train.HipSatTrainer.backward_batch, sat_train.HipSatTrainer.loss_and_grads,
               sat_train.loss_and_grads_through_tower, sat_train.train_step):
        assert inspect.signature(fn).parameters["batched"].default is False, fn.__name__


def test_begin_shapes_and_check_rows():
    """begin(): [T, 1024] (one sample, as before) or [B, T, 1024], d state fp32 of the same shape; check_rows(): the evaluation has
    one row per token set."""
    inj = _trainer().injector
    g = torch.zeros(8)
    B, T = 3, 9
    inj.begin(torch.zeros(B, T, 1024, dtype=torch.float16), g, torch.zeros(B, T, 1024))
    inj.check_rows(B)
    for rows in (B + 1, 1):
        with pytest.raises(ValueError, match=f"evaluates {rows} rows"):
            inj.check_rows(rows)
    inj.end()
    # B = 1 in the batched form is not the one-sample form, but holds one sample all the same
    inj.begin(torch.zeros(1, T, 1024, dtype=torch.float16), g, torch.zeros(1, T, 1024))
    inj.check_rows(1)
    with pytest.raises(ValueError):
        inj.check_rows(2)
    inj.end()
    # the one-sample form
    inj.begin(torch.zeros(T, 1024, dtype=torch.float16), g, torch.zeros(T, 1024))
    inj.check_rows(1)
    with pytest.raises(ValueError, match="1 sample, the UNet evaluates 3 rows"):
        inj.check_rows(3)
    inj.end()
    bad = [(torch.zeros(B, T, 1024), torch.zeros(B, T, 1024)),                                   # fp32 tokens
           (torch.zeros(B, T, 1000, dtype=torch.float16), torch.zeros(B, T, 1000)),              # not CLIP_DIM wide
           (torch.zeros(2, B, T, 1024, dtype=torch.float16), torch.zeros(2, B, T, 1024)),        # 4-D
           (torch.zeros(B, T, 1024, dtype=torch.float16), torch.zeros(T, 1024)),                 # d state of one sample
           (torch.zeros(B, T, 1024, dtype=torch.float16), torch.zeros(B, T, 1024, dtype=torch.float16))]
    for state, dstate in bad:
        with pytest.raises(AssertionError):
            inj.begin(state, g, dstate)


def test_forward_refuses_diff_from_with_shared_input():
    """The argument checks come first: a stand-in without a single attribute gets as far as them."""
    x = torch.zeros(2 * 64, 32, dtype=torch.float16)
    with pytest.raises(ValueError, match="shared_input"):
        HipUNet.forward(SimpleNamespace(), x, 5, 2, 8, None, shared_input=True, diff_from=0)
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="diff_from"):
            HipUNet.forward(SimpleNamespace(), x, 5, 2, 8, None, diff_from=bad)
