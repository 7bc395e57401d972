"""The record kernels of the output + loss and the two fused head launches (k_loss_rec, k_head_rec, k_latb_rec), read from the built
gfx950 code object (no GPU needed), as test_descriptor_codeobj.py reads k_small_desc and k_small_tn_desc.

They pay only if their leading kernel arguments -- the table pointer first -- arrive preloaded in SGPRs and no software division
stands between kernel entry and the first LDS-DMA.  Nothing else of the assembly is looked at."""
import re
import subprocess

from test_descriptor_codeobj import OBJDUMP, codeobj  # noqa: F401  (codeobj: the module-scoped fixture that extracts the code object)

NAMES = r"k_(loss|head|latb)_rec"


def kernels(syms):
    """mangled names of the record kernels' instances (functions in .text)"""
    out = [ln.split()[-1] for ln in syms.splitlines() if re.search(r"\sF\s+\.text\s", ln) and re.search(NAMES, ln)]
    # bf16 + fp32: one k_loss_rec, 5 transfer functions of k_head_rec and of k_latb_rec
    assert len(out) == 2 * (1 + 5 + 5), out
    return out


def test_leading_arguments_are_preloaded(codeobj):
    path, syms = codeobj
    for k in kernels(syms):
        kd = subprocess.run([OBJDUMP, "-D", "-j", ".rodata", "--disassemble-symbols=" + k + ".kd", path], capture_output=True, text=True,
                            check=True).stdout
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", kd)
        assert m, "no kernel descriptor of %s in:\n%s" % (k, kd[-1500:])
        # table pointer (2 SGPRs), stamps (2), launch id (1), the successor's lines (2), their count (1)
        assert int(m.group(1)) >= 8, (k, m.group(0))


def test_no_division_ahead_of_the_first_dma(codeobj):
    path, syms = codeobj
    for k in kernels(syms):
        dis = subprocess.run([OBJDUMP, "-d", "--disassemble-symbols=" + k, path], capture_output=True, text=True, check=True).stdout
        ins = [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]
        first = next((i for i, s in enumerate(ins) if s.startswith("global_load_lds")), None)
        assert first is not None, "no LDS-DMA in %s" % k
        assert not any(s.startswith("v_rcp_iflag_f32") for s in ins[:first]), (k, "software division ahead of the first DMA")
