"""What a stashing forward keeps, on the GPU (-m gpu): every tensor of unet.Stash holds exactly the differentiated rows - the last
rows - first batch rows - whichever launch produced it (all rows, the cond half of a shared CFG front, the rows a stashing launch
kept), and the backward reads the entries as they are."""
import pytest
import torch

from tests.test_gpu_sat_train import DEV, _rel, e2e  # noqa: F401 (fixture + harness)

pytestmark = pytest.mark.gpu

H = 16
PER_IMAGE = {"res": ("st1", "st2"), "tr": ("gst", "lse1", "lse2")}      # [batch rows, ...]; every other tensor is [batch rows * HW, ...]
# name: rows, timesteps, shared_input, diff_from
FORMS = {"rows2_shared": (2, 501, True, None), "rows2": (2, 501, False, None), "rows3_from1": (3, (37, 803, 411), False, 1),
         "rows3_from0": (3, (37, 803, 411), False, 0), "rows1": (1, 803, False, None)}
_WALKS = {}


def _check_entries(stash, S):
    """Every tensor of every entry holds S batch rows; every tensor key is present in every entry of its table."""
    n = 0
    for table, per_image in (("res", PER_IMAGE["res"]), ("tr", PER_IMAGE["tr"])):
        for p, ent in getattr(stash, table).items():
            HW = ent["sz"][0] * ent["sz"][1]
            assert "half" not in ent
            for k, v in ent.items():
                if not torch.is_tensor(v):
                    assert k in ("sz", "heads") or v is None, (p, k)
                    continue
                want = S if k in per_image else S * HW
                assert v.shape[0] == want, (table, p, k, tuple(v.shape), want)
                n += 1
    return n


def _walk(net, name):
    """The stashing forward of one form (computed once, shared, never modified): inputs from a fixed seed; the two rows = 2 forms get
    the same CFG-doubled latents."""
    if name not in _WALKS:
        from oracle import unet as ounet
        from sketch2img_amd import ops
        from sketch2img_amd.unet import CIN_PAD, Stash
        rows, ts, shared, diff_from = FORMS[name]
        g = torch.Generator().manual_seed(41)
        x1 = torch.randn(1, 4, H, H, generator=g)
        x = torch.cat([x1, x1]) if rows == 2 else torch.randn(rows, 4, H, H, generator=g)
        ehs = torch.randn(3, 77, ounet.TINY.cross_attention_dim, generator=g).half().float()[:rows]
        net.prepare_context(ehs)
        stash = Stash()
        kw = {} if diff_from is None else {"diff_from": diff_from}
        eps, taps = net.forward(ops.nchw_to_nhwc(x.to(DEV), CIN_PAD), list(ts) if isinstance(ts, tuple) else ts, rows, H, stash,
                                want_taps=True, want_eps=True, shared_input=shared, **kw)
        _WALKS[name] = dict(rows=rows, first=rows // 2 if diff_from is None else diff_from, stash=stash, eps=eps, taps=taps, ctx=net.ctx)
    return _WALKS[name]


@pytest.mark.parametrize("name", list(FORMS))
def test_stash_holds_the_differentiated_rows_and_the_backward_reads_them(e2e, name):
    """TINY UNet at 16 x 16 in the five forms a caller can ask for: every per-row tensor of every stash entry has (rows - first) * HW
    rows, every per-image tensor rows - first; backward_eps of a random seed (backward of random tap gradients for the shared CFG
    form, the sampler's call) returns a finite tensor of (rows - first) * HW rows."""
    from sketch2img_amd.unet import EPS_SEED_LD
    net = e2e["net"]
    w = _walk(net, name)
    rows, first, stash = w["rows"], w["first"], w["stash"]
    S = rows - first
    assert (stash.rows, stash.first) == (rows, first) and "rows" not in stash.misc and "diff_from" not in stash.misc
    assert len(stash.res) == 22 and len(stash.tr) == 16
    n = _check_entries(stash, S)
    assert n == 22 * 4 + 16 * 15, n
    assert stash.misc["out_h"].shape[0] == S * H * H and stash.misc["out_st"].shape[0] == S
    net.ctx = w["ctx"]
    g = torch.Generator().manual_seed(43)
    if FORMS[name][2]:
        grads = [(0.05 * torch.randn(S * (t.shape[0] // rows), t.shape[1], generator=g)).half().to(DEV) for t, _ in w["taps"]]
        dx = net.backward(stash, grads)
    else:
        seed = torch.zeros(S * H * H, EPS_SEED_LD, dtype=torch.float16, device=DEV)
        seed[:, :4] = torch.randn(S * H * H, 4, generator=g).half().to(DEV)
        dx = net.backward_eps(stash, seed)
    assert dx.shape[0] == S * H * H and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0.0


def test_shared_front_and_doubled_walk_keep_the_same_cond_row(e2e):
    """rows = 2, the same latents in both halves, with and without the shared CFG front: the stash entries - the cond row in both -
    are equal key by key where the two walks' outputs (eps, the nine taps) are equal bit for bit, the condition of
    test_gpu_pipeline.py::test_shared_cfg_prefix_is_bit_identical (the half-size launches then ran the same instantiations).  Where
    they are not, a key that differs is printed and skipped - never a key of stash.res: the resnets run the same instantiations at
    this size."""
    net = e2e["net"]
    a, b = _walk(net, "rows2_shared"), _walk(net, "rows2")
    same_out = torch.equal(a["eps"], b["eps"]) and all(torch.equal(u[0], v[0]) for u, v in zip(a["taps"], b["taps"]))
    skipped = []
    for table in ("res", "tr"):
        ta, tb = getattr(a["stash"], table), getattr(b["stash"], table)
        assert list(ta) == list(tb)
        for p in ta:
            assert list(ta[p]) == list(tb[p])
            for k, v in ta[p].items():
                if not torch.is_tensor(v):
                    assert v == tb[p][k], (p, k)
                elif not (v.shape == tb[p][k].shape and torch.equal(v, tb[p][k])):
                    assert table == "tr" and not same_out, (table, p, k, "differs although eps and taps are bit-equal")
                    skipped.append(f"{p}.{k}")
    print(f"[stash rows] shared vs doubled: outputs bit-equal {same_out}; skipped keys: {skipped or 'none'}")


def test_c320_block_stashing_launches_keep_the_cond_row(monkeypatch):
    """SD1.5's down_blocks.0.attentions.0 (C = 320, 8 heads; synthetic weights rounded to fp16) on rows = 2 at 16 x 16 with the
    default diff_from: the stashing launches run with keep_from = HW and the entry holds the cond row of every tensor; _tr_bwd of
    that row against autograd of oracle.unet.transformer2d_forward, d x within 2 x the fp16-storage emulation's distance (the
    harness and bound of test_gpu_sat_train_batched.py::test_c320_transformer_block_all_rows_stashed)."""
    from oracle import unet as ounet
    from sketch2img_amd import ops, synthetic
    from sketch2img_amd.config import SD15
    from sketch2img_amd.unet import HipUNet, Stash
    p, rows, hh, C, heads = "down_blocks.0.attentions.0", 2, 16, 320, 8
    HW = hh * hh
    W = {k: v.half().float() for k, v in synthetic.unet_state_dict(SD15).items() if k.startswith(p + ".")}
    net = HipUNet(SD15, W, DEV)
    g = torch.Generator().manual_seed(321)
    x = torch.randn(rows, C, hh, hh, generator=g).half().float()
    ehs = torch.randn(rows, 77, SD15.cross_attention_dim, generator=g).half().float()
    dout = (0.05 * torch.randn(rows, C, hh, hh, generator=g)).half().float()

    def run(emulate):
        xg = x.clone().requires_grad_(True)
        with ounet.fp16_storage(emulate):
            out = ounet.transformer2d_forward(ounet.SD15, W, p, xg, ehs, heads)
            (out[1:] * dout[1:]).sum().backward()
        return xg.grad[1:]

    ref, emu = run(False), run(True)
    calls = []
    for name in ("xattn_block", "ff_block_proj", "ff_block", "gemm_geglu_keep"):
        def counted(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append((_n, k.get("keep_from")))
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C).half().to(DEV).contiguous()
    net.prepare_context(ehs)
    stash = Stash(rows=rows, first=1)
    net._tr_fwd(p, tok(x), rows, (hh, hh), heads, stash)
    fused = [c for c in calls if c[0] in ("xattn_block", "ff_block_proj", "ff_block")]
    print(f"[C=320 block rows=2] launches: {calls} -> {'fused stashing' if fused else 'per-operator'}")
    assert calls and all(kf in (HW, None) for _, kf in calls) and all(kf == HW for _, kf in fused)
    assert list(stash.tr) == [p] and not stash.res
    assert _check_entries(stash, 1) == 15
    dx = net._tr_bwd(p, tok(dout[1:]), 1, stash.tr[p])
    got = dx.float().cpu().view(1, hh, hh, C).permute(0, 3, 1, 2)
    e, b = _rel(got, ref), 2 * _rel(emu, ref)
    print(f"[C=320 block rows=2] cond row d x: hip {e:.3e} bound {b:.3e}")
    assert e <= b, (e, b)
