"""CPU: instruction-level guards on the built gfx950 code (no GPU needed: the device code object is extracted from the in-tree object
file and disassembled with the ROCm LLVM tools).

ADVICE r3 / DESIGN "A nondeterminism that was NOT a wait-count problem": the first bf16 build of pw_bnbwd_dgrad2_kernel lost the addend
in a few lanes, differently from launch to launch; every failing build had the compiler's `v_pk_add_f32 ... op_sel:[0,1] op_sel_hi:[1,0]`
(swapped halves of the widened bf16 addend) in the store block behind the DPP transpose, no stable build had it.  No root cause was
found — it is an OPEN correctness risk — so the source spells those adds as scalar v_add_f32, and this test fails the build if the
compiler ever brings the packed form back in that kernel family (the run-to-run determinism tests in tests/test_gpu_kernels.py are the
behavioural guard)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
# counted in pwgemm.o of the last build before the split, with the code of this file: stage 1 4 fp32 + 2 bf16, finalize 1, first-generation
# data gradient 1, second generation 3 fp32 + 3 fp32 with sums + 5 bf16
PW_BNBWD_FUNCTIONS = 19


def _functions(obj, workdir):
    """{function symbol: [instruction text, ...]} of the gfx950 code object inside a host object file."""
    tools = [os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-objdump"), shutil.which("objcopy")]
    if not all(t and os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM binutils not found")
    stem = os.path.splitext(os.path.basename(obj))[0]
    fat, co = str(workdir / (stem + ".fat.bin")), str(workdir / (stem + ".co"))
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([tools[0], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co, "--unbundle"])
    txt = subprocess.run([tools[1], "-d", co], capture_output=True, text=True, check=True).stdout
    funcs, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur is not None:
            funcs[cur].append(line.split("//")[0])
    return funcs


@pytest.fixture(scope="module")
def pointwise_functions(tmp_path_factory):
    """The device functions of the five pointwise-GEMM units, per object."""
    import mobilenet_yolo_pytorch_amd.build as b
    b.build()
    d = tmp_path_factory.mktemp("isa")
    return {name: _functions(os.path.join(b.OBJ, name), d) for name in ("pwgemm.o", "pwntv1.o", "pwntred.o", "pwwgrad.o", "pwbnbwd.o")}


@pytest.fixture(scope="module")
def pwbnbwd_disassembly(pointwise_functions):
    return pointwise_functions["pwbnbwd.o"]


def test_bf16_stage2_kernels_have_no_swapped_packed_add(pwbnbwd_disassembly):
    bad_form = re.compile(r"v_pk_add_f32\b.*op_sel:\[0,1\] op_sel_hi:\[1,0\]")
    kernels = {k: v for k, v in pwbnbwd_disassembly.items() if "pw_bnbwd_dgrad2_kernel" in k and "bf16_t" in k}
    assert len(kernels) == 5, sorted(kernels)            # N = 64, 72, 96, 144, 192
    for name, body in kernels.items():
        assert len(body) > 500, name
        hits = [ln.strip() for ln in body if bad_form.search(ln)]
        assert not hits, (name, hits[:3])
        # the epilogue's addend adds are there, as scalar adds behind the DPP quad transpose
        assert any("v_add_f32" in ln for ln in body) and any("row_shr" in ln or "quad_perm" in ln or "dpp" in ln.lower() for ln in body), name


def test_every_pointwise_kernel_family_is_compiled_in_one_unit(pointwise_functions):
    """csrc/pwgemm.hip was split by kernel family so that the families compile side by side.  A family instantiated in two units would compile
    twice and nothing else would show it: every symbol is in one object, every family in its own, in the numbers of the tables."""
    where = {}
    for obj, funcs in pointwise_functions.items():
        for sym in funcs:
            where.setdefault(sym, []).append(obj)
    assert not {s: o for s, o in where.items() if len(o) > 1}

    def count(family):      # {object: functions of the family}; the mangled name holds <length><name>
        out = {}
        for sym, objs in where.items():
            if re.search(r"\d%s(?![a-z0-9_])" % family, sym):
                out[objs[0]] = out.get(objs[0], 0) + 1
        return out

    wg = {f: count(f) for f in ("pw_wgrad_kernel", "pw_wgrad_dma_kernel", "pw_wgrad_bf16_kernel")}
    assert all(set(c) == {"pwwgrad.o"} for c in wg.values()), wg
    assert sum(c["pwwgrad.o"] for c in wg.values()) == 113, wg          # 36 + 23 + 54 (tests/wgrad_regimes.py ROWS)
    assert count("pw_bnbwd_[a-z0-9_]*") == {"pwbnbwd.o": PW_BNBWD_FUNCTIONS}
    assert count("pw_gemm_nt_kernel") == {"pwntv1.o": 16}               # 2 storage types x 4 column tiles x 2 BK
    assert count("pw_gemm_nt_dma_kernel") == {"pwgemm.o": 60, "pwntred.o": 43}
    assert sum(count("reduce_parts_kernel").values()) == 1
