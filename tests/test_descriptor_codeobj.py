"""The descriptor kernels' prologue, read from the built gfx950 code object (no GPU needed).

k_small_desc and k_small_tn_desc are worth having only if (a) their leading kernel arguments -- the table pointer first -- arrive
preloaded in SGPRs (the build's -amdgpu-kernarg-preload-count) and (b) nothing stands between kernel entry and the first LDS-DMA
but one wait for the record: no software division, no chain of scalar round trips.  Both are properties of the compiled code, so
they are checked there: the kernel descriptors and the disassembly of libavae.so's embedded code object.  (The chain's other three
kernels -- k_small_loss, k_small_head, k_small_latb -- keep their by-value items and are not looked at here.)"""
import os
import re
import struct
import subprocess

import pytest

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


@pytest.fixture(scope="module")
def codeobj(tmp_path_factory):
    """path of the gfx950 code object that holds the small-net kernels, and its symbol table"""
    if not os.path.exists(OBJDUMP):
        pytest.fail("llvm-objdump of the ROCm toolchain is needed to read the code object")
    import __graft_entry__ as g
    g.build()
    data = open(g.LIB, "rb").read()
    d = tmp_path_factory.mktemp("codeobj")
    pos = 0
    while True:                       # one offload bundle per translation unit: [magic][n][(offset, size, id length, id) x n]
        i = data.find(MAGIC, pos)
        assert i >= 0, "no gfx950 code object with the descriptor kernels in " + g.LIB
        n, = struct.unpack_from("<Q", data, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, idl = struct.unpack_from("<QQQ", data, p)
            tid = data[p + 24:p + 24 + idl].decode()
            p += 24 + idl
            if "gfx950" in tid and size and b"k_small_tn_desc" in data[i + off:i + off + size]:
                path = str(d / "kernels.co")
                with open(path, "wb") as f:
                    f.write(data[i + off:i + off + size])
                syms = subprocess.run([OBJDUMP, "-t", path], capture_output=True, text=True, check=True).stdout
                return path, syms
        pos = i + len(MAGIC)


def kernels(syms):
    """mangled names of the descriptor kernels' instances (functions in .text)"""
    out = [ln.split()[-1] for ln in syms.splitlines() if re.search(r"\sF\s+\.text\s", ln) and re.search(r"k_small_(tn_)?desc", ln)]
    # bf16 + fp32: 2 kinds x 5 transfer functions of k_small_desc, one k_small_tn_desc
    assert len(out) == 2 * (2 * 5 + 1), out
    return out


def test_leading_arguments_are_preloaded(codeobj):
    path, syms = codeobj
    for k in kernels(syms):
        kd = subprocess.run([OBJDUMP, "-D", "-j", ".rodata", "--disassemble-symbols=" + k + ".kd", path], capture_output=True, text=True,
                            check=True).stdout
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", kd)
        assert m, "no kernel descriptor of %s in:\n%s" % (k, kd[-1500:])
        # table pointer (2 SGPRs), stamps (2), launch id (1), the successor's records (2), their count (1)
        assert int(m.group(1)) >= 8, (k, m.group(0))


def test_prologue_is_one_burst(codeobj):
    path, syms = codeobj
    for k in kernels(syms):
        dis = subprocess.run([OBJDUMP, "-d", "--disassemble-symbols=" + k, path], capture_output=True, text=True, check=True).stdout
        ins = [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]
        first = next((i for i, s in enumerate(ins) if s.startswith("global_load_lds")), None)
        assert first is not None, "no LDS-DMA in %s" % k
        pro = ins[:first]
        assert not any(s.startswith("v_rcp_iflag_f32") for s in pro), (k, "software division ahead of the first DMA")
        # one in the entry sequence for loaders that do not preload (it is skipped when they do), one for the record
        waits = [s for s in pro if s.startswith("s_waitcnt") and "lgkmcnt" in s]
        assert len(waits) <= 2, (k, waits)
