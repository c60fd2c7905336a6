"""CPU: the MXFP8 rule of tests/kv_mxfp8_checks.py against torch.float8_e4m3fn of x / 2^e and against hand cases; x_hat exact and a fixed point; the header, the
binding, the library and INTEGRATION.md agree on ABI 21 and the two symbols; both entry points refuse bad arguments before any launch; generate() refuses bad
kv_format / kv_cache before anything touches a device."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

from tests import kv_mxfp8_checks as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
SYMS = ("llmseg_kv_quantize_mxfp8", "llmseg_decode_attn_mxfp8")


def _block(values, fill=0.0):
    x = torch.full((1, 32), fill)
    x[0, :len(values)] = torch.tensor(values, dtype=torch.float32)
    return x.to(BF)


# ------------------------------------------------------------------------------------------------------------------------------------ the rule
def test_rule_against_float8_e4m3fn_on_random_blocks():
    x = torch.cat([kc.blocks(4096, 1), (kc.blocks(2048, 2).float() * 2.0 ** -60).to(BF), (kc.blocks(2048, 3).float() * 2.0 ** 60).to(BF)])
    q, sb, xh = kc.quantize(x)
    assert q.dtype == torch.uint8 and sb.dtype == torch.uint8 and xh.dtype == BF and sb.shape == (x.shape[0], 1)
    e = sb.view(-1).double() - 127
    amax = x.double().abs().amax(-1)
    assert bool((amax <= 448 * 2 ** e).all()), "a block saturates under its scale"
    assert bool(((e == -127) | (amax > 448 * 2 ** (e - 1))).all()), "e is not the smallest admissible exponent"
    assert int(sb.max()) <= 247
    code, xh_ref = kc.float8_reference(x, sb)
    assert not bool(((code & 0x7F) == 0x7F).any()), "torch.float8_e4m3fn of y holds a NaN"
    assert torch.equal(q, code), f"{int((q != code).sum())} codes differ from torch.float8_e4m3fn(x / 2^e)"
    normal = sb.view(-1) > 9                                 # every x_hat of such a block is a normal bf16 or zero
    assert int(normal.sum()) > 6000                    # (one block in eight is all zero)
    assert torch.equal(xh.double()[normal], xh_ref[normal]), "x_hat is not element * 2^e exactly"
    assert bool(((xh.double() - x.double()).abs() <= 2.0 ** -4 * amax[:, None])[normal].all())
    assert not bool(((q == 0x80)).any()), "-0 was stored"


def test_hand_cases():
    z = kc.quantize(_block([]))
    assert int(z[1]) == 0 and not bool(z[0].any()) and not bool(kc.bits(z[2]).any())           # all zero: e = -127, scale byte 0
    for k in (-20, -3, 0, 5, 30):
        s = 2.0 ** k
        q, sb, xh = kc.quantize(_block([448.0 * s, -1.0 * s]))                                # amax = 448 * 2^k: e = k, y = 448 = code 0x7e
        assert int(sb) == k + 127 and int(q[0, 0]) == 0x7E and float(xh[0, 0]) == 448.0 * s and int(q[0, 1]) == (0x80 | 0x38)
        q, sb, xh = kc.quantize(_block([1.7578125 * 256 * s]))                                # the next bf16 above it: e = k + 1, y = 225 -> 224
        assert int(sb) == k + 128 and int(q[0, 0]) == 0x76 and float(xh[0, 0]) == 448.0 * s
        # ties go to the even code: 1.0625 -> 1.0, 1.1875 -> 1.25, 2^-10 -> 0, 3 * 2^-10 -> 2^-8; amax = 256 * 2^k: e = k
        q, sb, xh = kc.quantize(_block([256.0 * s, 1.0625 * s, 1.1875 * s, 2.0 ** -10 * s, 3 * 2.0 ** -10 * s, -(2.0 ** -10) * s, 2.0 ** -9 * s, -0.0]))
        assert int(sb) == k + 127
        assert q[0, :8].tolist() == [0x78, 0x38, 0x3A, 0x00, 0x02, 0x00, 0x01, 0x00], q[0, :8].tolist()
        assert xh[0, :8].float().tolist() == [256.0 * s, 1.0 * s, 1.25 * s, 0.0, 2.0 ** -8 * s, 0.0, 2.0 ** -9 * s, 0.0]
        assert kc.bits(xh)[0, [3, 5, 7]].tolist() == [0, 0, 0], "a zero kept its sign"
    # subnormal elements beside a large amax: y is far below 2^-10
    q, sb, xh = kc.quantize(_block([100.0, 2.0 ** -133, -(2.0 ** -130), 2.0 ** -126, 2.0 ** -3, 2.0 ** -10]))
    assert int(sb) == 127 - 2 and q[0, :6].tolist() == [0x7C, 0, 0, 0, 0x30, 0x02]              # e = -2: y = 400 is a tie of the top binade (quantum 32) -> 384; 2^-1; 2^-8
    # a block of bf16 subnormals: e = -127 and y = x * 2^127 is on the E4M3 grid for small integers
    q, sb, _ = kc.quantize(_block([3 * 2.0 ** -133, -(2.0 ** -133)]))
    assert int(sb) == 0 and q[0, :2].tolist() == [0x14, 0x80 | 0x08]                           # 3 * 2^-6 = 1.5 * 2^-5, 2^-6


def test_x_hat_is_a_fixed_point():
    """A second quantisation of x_hat gives x_hat again, bit for bit, and the same bytes and scale bytes wherever the block's scale is derived anew as it was.
    It is NOT always: a block whose amax was rounded DOWN onto 1.75 * 2^E (y in (224, 232] -> 224, the code 0x76 under e = E - 7) meets the rule's other branch the
    second time (m = 1.75: e = E - 8), so its scale byte drops by one and every code moves up one binade -- the same values in other bytes."""
    x = torch.cat([kc.blocks(4096, 11), kc.blocks(512, 12)])
    q, sb, xh = kc.quantize(x)
    q2, sb2, xh2 = kc.quantize(xh)
    normal = sb.view(-1) > 9
    assert torch.equal(kc.bits(xh2)[normal], kc.bits(xh)[normal])
    top = (q & 0x7F).amax(-1) == 0x76
    same = sb2.view(-1) == sb.view(-1)
    assert torch.equal(q2[same & normal], q[same & normal])
    assert bool((same | top | ~normal).all()), "a scale byte moved on a block whose amax code is not 0x76"
    assert bool((sb2.view(-1)[top & normal].int() == sb.view(-1)[top & normal].int() - 1).all())
    assert 0 < int(top.sum()) < x.shape[0] // 4                       # (one block kind in eight aims at it)
    assert torch.equal(kc.bits(kc.dequantize(q, sb)), kc.bits(xh))


# ------------------------------------------------------------------------------------------------------------------ header, binding, library
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmseg_hip.h")).read(), flags=re.S)


def test_symbols_are_declared_bound_exported_and_documented_at_abi_21():
    from llmseg_amd import _lib
    src = _header()
    abi = int(re.search(r"#define LLMSEG_ABI_VERSION (\d+)", src).group(1))
    assert abi == _lib.ABI_VERSION >= 21
    lib = _lib.load()
    assert lib.llmseg_version() == abi
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"llmseg_version\(\) == %d\b" % abi, doc)
    for sym in SYMS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, src), f"{sym} is not declared in include/llmseg_hip.h"
        decl = re.search(r"%s\s*\((.*?)\)\s*;" % sym, src, flags=re.S).group(1).split(",")
        kinds = [C.c_void_p if "*" in a else C.c_float if "float" in a else C.c_int32 if "int32_t" in a else C.c_int64 for a in decl]
        assert _lib.SIGNATURES[sym] == kinds, sym
        assert hasattr(lib, sym) and sym in doc
    assert "kv_quant.hip" in open(os.path.join(ROOT, "llmseg_amd", "csrc", "build.sh")).read()
    full = open(os.path.join(ROOT, "include", "llmseg_hip.h")).read()
    assert "448 * 2^e" in full and "E8M0" in full and "scale[n][t][h * 4 + d / 32]" in full


def test_kv_quantize_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    ok = dict(x=4096, xb=4096, xr=256, q=8192, qb=4096, qr=256, s=16384, sb=128, sr=8, h=32768, hb=4096, hr=256, row0=65536, r0s=1, batch=2, rows=16, D=256)
    bads = [dict(x=None), dict(x=4104), dict(q=None), dict(s=None), dict(q=None, s=None, h=None), dict(q=8196), dict(h=32776), dict(row0=65538), dict(r0s=2), dict(r0s=-1),
            dict(D=0), dict(D=48), dict(D=-32), dict(batch=0), dict(rows=0), dict(rows=-1), dict(xr=248), dict(xr=260), dict(qr=128), dict(qr=260), dict(sr=7), dict(hr=128),
            dict(xb=2048), dict(qb=2048), dict(sb=64), dict(hb=2048), dict(xb=4100)]
    n0 = lib.llmseg_launch_count()
    for bad in bads:
        a = dict(ok, **bad)
        rc = lib.llmseg_kv_quantize_mxfp8(p(a["x"]), a["xb"], a["xr"], p(a["q"]), a["qb"], a["qr"], p(a["s"]), a["sb"], a["sr"], p(a["h"]), a["hb"], a["hr"], p(a["row0"]), a["r0s"],
                                          a["batch"], a["rows"], a["D"], None)
        assert rc == -1 and b"kv_quantize_mxfp8" in lib.llmseg_last_error(), bad
    assert lib.llmseg_launch_count() == n0


def test_decode_attn_mxfp8_refuses_bad_arguments_before_any_launch():
    from llmseg_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    ok = dict(qkv=4096, ld=768, cos=4096, sin=4096, kc=8192, vc=8192, cs=65536, ks=4096, vs=4096, ss=2048, pos=4096, ps=1, src=4096, ld_src=256, cap=256, N=2, heads=2, hd=128,
              out=4096, scratch=None)
    bads = [dict(qkv=None), dict(cos=None), dict(sin=None), dict(kc=None), dict(vc=None), dict(ks=None), dict(vs=None), dict(pos=None), dict(out=None), dict(N=0), dict(N=65536),
            dict(heads=0), dict(hd=64), dict(qkv=4104), dict(ld=772), dict(kc=8196), dict(vc=8196), dict(cs=65540), dict(cs=128), dict(ks=4098), dict(vs=4097), dict(ss=2050),
            dict(ss=4), dict(ps=2), dict(ps=-1), dict(src=4098), dict(ld_src=128), dict(cap=0)]
    n0 = lib.llmseg_launch_count()
    for bad in bads:
        a = dict(ok, **bad)
        rc = lib.llmseg_decode_attn_mxfp8(p(a["qkv"]), a["ld"], p(a["cos"]), p(a["sin"]), p(a["kc"]), p(a["vc"]), a["cs"], p(a["ks"]), p(a["vs"]), a["ss"], p(a["pos"]), a["ps"],
                                          p(a["src"]), a["ld_src"], a["cap"], a["N"], a["heads"], a["hd"], 0.088, p(a["out"]), 256, p(a["scratch"]), 0, None)
        assert rc == -1 and b"decode_attn_mxfp8" in lib.llmseg_last_error(), bad
    assert lib.llmseg_launch_count() == n0


# ------------------------------------------------------------------------------------------------------------------ generate(), evaluate(), ops
def test_signatures_carry_the_defaults():
    from llmseg_amd import ops
    from llmseg_amd.generate import GenerateMixin
    from llmseg_amd.sam_decoder import SamDecoderMixin
    gen, ev = inspect.signature(GenerateMixin.generate).parameters, inspect.signature(SamDecoderMixin.evaluate).parameters
    assert gen["kv_format"].default is None and ev["kv_format"].default is None and gen["kv_cache"].default == "packed"
    da = inspect.signature(ops.decode_attn).parameters
    assert list(da)[-2:] == ["k_scale", "v_scale"] and da["k_scale"].default is None and da["v_scale"].default is None
    assert callable(ops.kv_quantize_mxfp8)


def test_generate_refuses_bad_kv_arguments_before_touching_a_device():
    """the checks come before prepare(): a stand-in for `self` that has a config and nothing else is enough"""
    from llmseg_amd.generate import GenerateMixin

    def stub(head_dim=128, hidden=256):
        return types.SimpleNamespace(config=types.SimpleNamespace(llama=types.SimpleNamespace(vocab=100, head_dim=head_dim, hidden=hidden)), _ragged_prompts=GenerateMixin._ragged_prompts)
    ids = torch.zeros((2, 6), dtype=torch.int64)
    ids[:, 1] = -200
    gen = lambda st=None, **kw: GenerateMixin.generate(st or stub(), None, ids, max_new_tokens=4, **kw)
    for bad in ("fp8", "mxfp4", 8, True, ""):
        with pytest.raises(ValueError, match="kv_format"):
            gen(kv_format=bad)
    for bad in ("copy", None, "fp8", 0):
        with pytest.raises(ValueError, match="kv_cache"):
            gen(kv_format="mxfp8", kv_cache=bad)
    with pytest.raises(ValueError, match="needs kv_format"):
        gen(kv_cache="bf16")
    with pytest.raises(ValueError, match="fuse_decode"):
        gen(kv_format="mxfp8", fuse_decode=False)
    with pytest.raises(ValueError, match="fuse_decode"):
        gen(kv_format="mxfp8", kv_cache="bf16", fuse_decode=False)
    with pytest.raises(ValueError, match="head_dim 128"):
        gen(stub(head_dim=64), kv_format="mxfp8")
    with pytest.raises(ValueError, match="hidden % 32"):
        gen(stub(hidden=128 + 16), kv_format="mxfp8")
    with pytest.raises(ValueError, match="num_beams"):                     # what the pinned refusals refuse is unchanged
        gen(kv_format="mxfp8", num_beams=2, do_sample=True)
