"""Resources of every transformer kernel instantiation, read from the compiler's own assembly for gfx950 (no GPU
needed): no instantiation touches scratch, each stays within the 160 KiB of LDS of a CU (the residency it is launched
for: k_tfm_ffn<C >= 256> and k_tfm_attn<64> run one workgroup per CU), and the kernels of the d = 96 / 3-head trunk keep
the VGPR and LDS figures they had before other widths existed."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
SOURCES = ["transformer.hip", "transformer.h", "transformer_core.h", "transformer_qkv_body.inc",
           "transformer_attn_body.inc", "transformer_ffn_body.inc"]
LDS_PER_CU = 160 * 1024
WIDTHS = [64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384]
# (VGPRs incl. AGPRs, LDS bytes) of the b14d96h3_transformer kernels as first built
D96 = {("qkv", 96, 32): (136, 13312), ("attn", 32): (308, 55808), ("ffn", 96): (248, 63744)}


def _assembly():
    h = hashlib.sha256()
    for f in SOURCES:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    out = os.path.join(ROOT, "build", "transformer_gfx950_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                            os.path.join(CSRC, "transformer.hip"), "-o", out + ".tmp"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".tmp", out)
    return open(out).read()


def _key(symbol):
    m = re.match(r"_ZN2p312_GLOBAL__N_1\d+k_tfm_(qkv|attn|ffn)ILi(\d+)E(?:Li(\d+)E)?EEvNS_\d+Tfm\w+ArgsE$", symbol)
    assert m, symbol
    return (m.group(1),) + tuple(int(g) for g in m.groups()[1:] if g is not None)


@pytest.fixture(scope="module")
def kernels():
    """{("qkv", C, D) | ("attn", D) | ("ffn", C): (vgpr + agpr count, LDS bytes, scratch bytes)}"""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    res = {}
    for b in _assembly().split("  - .agpr_count:")[1:]:
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1))
        res[_key(re.search(r"\.name:\s+(\S+)", b).group(1))] = (g("vgpr_count"), g("group_segment_fixed_size"),
                                                              g("private_segment_fixed_size"))
    return res


def test_every_supported_width_has_its_kernels(kernels):
    want = {("qkv", c, d) for c in WIDTHS for d in (32, 64) if c % d == 0} | {("attn", 32), ("attn", 64)} | \
        {("ffn", c) for c in WIDTHS}
    assert set(kernels) == want


def test_no_instantiation_uses_scratch_or_more_lds_than_a_cu_has(kernels):
    for key, (vgpr, lds, scratch) in kernels.items():
        assert scratch == 0, key
        assert lds <= LDS_PER_CU, (key, lds)
        assert vgpr <= 512, (key, vgpr)


def test_d96h3_kernels_keep_their_figures(kernels):
    for key, (vgpr, lds) in D96.items():
        assert kernels[key][:2] == (vgpr, lds), (key, kernels[key])
