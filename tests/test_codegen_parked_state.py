"""What the timed eye megakernels carry across the traversal pass (csrc/eye_kernel_body.h), read from the gfx950 code object the
library holds -- as tests/test_codegen_guard.py reads it, without a GPU.  The kernel sits at 128 VGPRs and spills path state that is
parked across trace_pool; the spill stores are nearly all of its writes to HBM.  Since the pixel coordinates travel as one word and a
batched launch parks a finished path's radiance in its frame's film instead of three registers, the private segment of the timed
forms is pinned here at what that reached:
    form                     before     now
    single frame, plain      128 B      128 B
    single frame, general    144 B      128 B
    batched, plain           144 B      128 B      (bench.py's kernel)
    batched, general         160 B      128 B
A lower spill must not be bought with reloads inside the traversal loop: SGPRs are at their limit too, and a spilled SGPR comes
back through v_readlane_b32.  READLANES_BEFORE is the count of those inside the traversal loop of each form in the build of the
commit before this change (tools/loop_mix.py --all on that build's libspcbpt_hip.so: 31 / 8 / 31 / 19); no form may hold more."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
ARGS = "EEEvNS_7KParamsE"
# <COUNT = false, BATCH, CACHE = true, ENV>: (symbol, private segment pinned [B], v_readlane_b32 in the traversal loop before this change)
FORMS = {"single frame, plain scene": ("_ZN3spc8k_spcbptILb0ELb0ELb1ELb0" + ARGS, 128, 31),
         "batched, plain scene (bench.py)": ("_ZN3spc8k_spcbptILb0ELb1ELb1ELb0" + ARGS, 128, 8),
         "single frame, general scene": ("_ZN3spc8k_spcbptILb0ELb0ELb1ELb1" + ARGS, 128, 31),
         "batched, general scene": ("_ZN3spc8k_spcbptILb0ELb1ELb1ELb1" + ARGS, 128, 19)}


def _traversal_loop(ins):
    """The pooled traversal loop of one kernel: the smallest backward branch's span that holds the pool cursor's ds_add_rtn_u32, the slab
    test's v_pk_fma_f32 and at least four 16-byte record fetches (the definition of tests/test_codegen_guard.py).  `ins` is
    [(address, mnemonic, branch target or None)]; returns the mnemonics inside the loop."""
    idx = {a: i for i, (a, _, _) in enumerate(ins)}
    best = None
    for i, (a, op, tgt) in enumerate(ins):
        if tgt is None or tgt > a or tgt not in idx:
            continue
        ops = [ins[k][1] for k in range(idx[tgt], i + 1)]
        if "ds_add_rtn_u32" in ops and "v_pk_fma_f32" in ops and sum("_load_dwordx4" in o for o in ops) >= 4:
            if best is None or len(ops) < len(best):
                best = ops
    return best


@pytest.fixture(scope="module")
def kernels(hip_lib, pkg, tmp_path_factory):
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf not present")
    d = tmp_path_factory.mktemp("co_parked")
    lib = shutil.copy(pkg.api.LIB_PATH, d)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    wanted = {sym for sym, _, _ in FORMS.values()}
    out = {}
    for f in sorted(os.listdir(d)):
        if "amdgcn-amd-amdhsa--gfx950" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(d, f)], stdout=subprocess.PIPE, text=True, check=True).stdout
        if "k_spcbpt" not in notes:
            continue
        for blk in notes.split("  - .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if name in wanted:
                out[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", os.path.join(d, f)], stdout=subprocess.PIPE, text=True, check=True).stdout
        cur, base, ins = None, None, {}
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur, base = (m.group(1), None) if m.group(1) in wanted else (None, None)
                continue
            m = cur and re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*(.*)$", line)
            if m:
                a = int(m.group(3), 16)
                if base is None:
                    base = a
                t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", m.group(4))
                ins.setdefault(cur, []).append((a, m.group(1), int(t.group(1), 16) + base if t else None))
        for name, body in ins.items():
            out[name]["loop"] = _traversal_loop(body)
    assert set(out) == wanted, sorted(wanted - set(out))
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_state_parked_across_the_traversal_pass(kernels, form):
    sym, scratch, readlanes_before = FORMS[form]
    k = kernels[sym]
    loop = k["loop"]
    report = {"form": form, "private_segment": k["private_segment_fixed_size"], "vgpr_spill_count": k["vgpr_spill_count"],
              "loop": len(loop) if loop else None, "v_readlane_b32 in loop": loop.count("v_readlane_b32") if loop else None}
    print(report)
    assert k["vgpr_count"] <= 128, report
    assert k["private_segment_fixed_size"] <= scratch, report
    assert loop, report
    assert loop.count("v_readlane_b32") <= readlanes_before, report
    assert not any(o.startswith("scratch_store") for o in loop), report
