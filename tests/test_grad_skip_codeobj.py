"""The two instances of the descriptor wgrad+adam launch, read from the built gfx950 code object (no GPU needed).

k_small_tn_desc stores the gradient, k_small_tn_nograd is the same body without that store (avae_kernels.hip: small_tn_desc_body).
The second one is worth having only if it keeps the first one's prologue -- preloaded leading arguments, one burst for the record
-- and costs no registers: checked on the kernel descriptors and the disassembly, as test_descriptor_codeobj.py does."""
import re
import subprocess

import pytest

from test_descriptor_codeobj import OBJDUMP, codeobj  # noqa: F401  (the fixture)


def instances(syms, name):
    out = sorted(ln.split()[-1] for ln in syms.splitlines() if re.search(r"\sF\s+\.text\s", ln) and re.search(name + r"I", ln))
    assert len(out) == 2, (name, out)         # bf16 and fp32, in the same order for both kernels (the mangled element type sorts them)
    return out


def descriptor(path, k):
    kd = subprocess.run([OBJDUMP, "-D", "-j", ".rodata", "--disassemble-symbols=" + k + ".kd", path], capture_output=True, text=True,
                        check=True).stdout
    field = lambda f: int(re.search(r"\.amdhsa_" + f + r"\s+(\d+)", kd).group(1))
    return dict(vgpr=field("next_free_vgpr"), sgpr=field("next_free_sgpr"), scratch=field("private_segment_fixed_size"),
                preload=field("user_sgpr_kernarg_preload_length"))


def code(path, k):
    dis = subprocess.run([OBJDUMP, "-d", "--disassemble-symbols=" + k, path], capture_output=True, text=True, check=True).stdout
    return [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]


def test_both_instances_no_scratch_no_more_registers(codeobj):
    path, syms = codeobj
    for keep, skip in zip(instances(syms, "k_small_tn_desc"), instances(syms, "k_small_tn_nograd")):
        a, b = descriptor(path, keep), descriptor(path, skip)
        print(keep, a, skip, b)
        assert a["scratch"] == 0 and b["scratch"] == 0, (a, b)
        assert b["vgpr"] <= a["vgpr"], (a, b)
        assert b["preload"] >= 8, b


def test_nograd_prologue_and_stores(codeobj):
    path, syms = codeobj
    for keep, skip in zip(instances(syms, "k_small_tn_desc"), instances(syms, "k_small_tn_nograd")):
        ins = code(path, skip)
        first = next(i for i, s in enumerate(ins) if s.startswith("global_load_lds"))
        pro = ins[:first]
        assert not any(s.startswith("v_rcp_iflag_f32") for s in pro), skip
        assert len([s for s in pro if s.startswith("s_waitcnt") and "lgkmcnt" in s]) <= 2, skip
        stores = lambda xs: len([s for s in xs if s.startswith("global_store") or s.startswith("flat_store")])
        # same K loop (as many LDS-DMAs), fewer stores: the gradient's
        assert len([s for s in ins if s.startswith("global_load_lds")]) == len([s for s in code(path, keep) if s.startswith("global_load_lds")])
        assert stores(ins) < stores(code(path, keep)), (skip, stores(ins), stores(code(path, keep)))
