"""Run as a script (subprocess of test_gpu_attention_fwd.py::test_env_variants) with SKG_ATTN_VAR or SKG_NO_ATTN_SHORT set: libskg.so
reads the switches once per process.  Asserts through skg_attn_fwd_variant that the switch moves the dh = 40 / 64 cases of
tests/attn_emulation.py to the instantiation it stands for, then runs the unit parity (the bounds of test_forward_parity) and the
one-hot / coded probes on them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketch2img_amd import ops  # noqa: E402
from tests import attn_emulation as ae  # noqa: E402
from tests.test_gpu_attention_fwd import onehot_probe, parity_fails, variant_of  # noqa: E402

VAR = os.environ.get("SKG_ATTN_VAR", "")
NO_SHORT = "SKG_NO_ATTN_SHORT" in os.environ
SMALL40 = ["rowv40", "vt40", "vt40_77", "rowv40_t5"]
LARGE40 = ["qt3_xcd", "qt3_xcd_vt", "qt3_plain", "qt3_wave"]
ROW64, VT64 = ["rowv64", "rowv64_t5"], ["vt64"]
# case or probe name -> (variant, queries per workgroup) under this process's switch
if NO_SHORT:      # the 77-key and the resident cases run the streaming kernel: QT 3 at dh 40 where the launch has 1024 workgroups of 192
    CASES = {"short40_q64": (1002, 128), "short40_k50": (1002, 128), "short40_k80": (1002, 128), "short40_q192": (1003, 192),
             "short64_q128": (1002, 128), "res10_40": (1002, 128), "res15_64": (1002, 128)}
    PROBES = {"short40": (1002, 128), "short64": (1002, 128), "res10_40": (1002, 128)}
elif VAR == "9":
    CASES = dict({n: (1003, 192) for n in SMALL40 + LARGE40}, rowv64=(1002, 128))
    PROBES = {"rowv40": (1003, 192), "vt40": (1003, 192), "qt3": (1003, 192)}
elif VAR == "8":
    CASES = dict({n: (1004, 256) for n in ROW64}, vt64=(1002, 128), rowv40=(1002, 128))
    PROBES = {"rowv64": (1004, 256), "vt64": (1002, 128)}
elif VAR == "12":
    CASES = dict({n: (1002, 128) for n in SMALL40 + LARGE40}, rowv64=(1002, 128))
    PROBES = {"qt3": (1002, 128), "rowv40": (1002, 128)}
elif VAR == "7":      # the same code as shipped (QT 2), the two-register-set instantiation behind it
    CASES = {n: (1002, 128) for n in ROW64 + VT64}
    PROBES = {"rowv64": (1002, 128), "vt64": (1002, 128)}
else:
    raise SystemExit("set SKG_ATTN_VAR to 7, 8, 9 or 12, or SKG_NO_ATTN_SHORT")

fails = []
for name, expect in CASES.items():
    c = ae.FWD_BY_NAME[name]
    got = variant_of(ops, c)
    if got != expect:
        fails.append(f"{name}: skg_attn_fwd_variant reports {got}, expected {expect}")
        continue
    q, k, v = ae.fwd_inputs(c, "unit")
    r = ae.emulate_forward(q, k, v, c.heads, c.dh ** -0.5, bool(c.flags & ae.CAUSAL), ae.fwd_denom_fp16(got[0], c.dh))
    fails += [f"{name}: {f}" for f in parity_fails(ops, c, "unit", (q, k, v), r, f"{name} dh{c.dh} b{c.B} {c.Nq}x{c.Nkv}/{c.kvs}")]
    sys.stdout.flush()
for name, expect in PROBES.items():
    try:
        onehot_probe(ops, {g.name: g for g in ae.FWD_PROBES}[name], expect)
        print(f"probe {name}: ok", flush=True)
    except AssertionError as e:
        fails.append(f"probe {name}: {e}")

print("FAILED: " + "; ".join(fails) if fails else "ALL OK")
sys.exit(1 if fails else 0)
