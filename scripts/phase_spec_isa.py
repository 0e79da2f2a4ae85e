#!/usr/bin/env python3
"""What the phase-specialised half-step instance (kmc_kernels.hpp: Spec::Credit) did to the gfx950 code: writes profiles/phase_spec_isa.txt.

Every kmc_inst_*.hip of this tree and of a parent commit is compiled to assembly (`hipcc -S --cuda-device-only`, the build's flags; no GPU needed).
  * Kernels both trees have -- every vector, generic, generation, island, resident ... instance -- are compared text against text: comment, .loc,
    .file and .ident lines, the per-unit __hip_cuid_* symbol and trailing comments left out, block labels renumbered.  Units whose kernels are all
    identical get one line; a kernel that differs is named.
  * Kernels only this tree has (the instances of kmc_inst_<density>_spec.hip) are listed with their static instruction counts by class and
    their VGPRs, next to the generic kernel of the same geometry.

    python scripts/phase_spec_isa.py [--parent REV] [--jobs N] [-o profiles/phase_spec_isa.txt]
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import importlib.util
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kissmcmc.jl_amd")


def build_module():
    spec = importlib.util.spec_from_file_location("kmc_build", os.path.join(PKG, "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def compile_asm(hipcc, flags, src, out):
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", src, "-o", out])
    return out


LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?")


def kernels_of(path):
    """name -> normalised text (body + kernel descriptor) of every kernel in an assembly file."""
    out, cur, name, dcur = {}, None, None, None
    desc = {}
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].rstrip()
            s = line.strip()
            if not s or s.startswith((".loc", ".file", ".ident", ".cfi_", ".p2align", ".section", ".text", ".protected", ".globl", ".weak", ".type", ".size")) or "__hip_cuid_" in s:
                continue
            s = LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), s)
            m = re.match(r"^(_Z\w+):$", s)
            if m and cur is None:
                name, cur = m.group(1), []
            elif s.startswith(".amdhsa_kernel "):          # (the descriptor stands inside its kernel's function, ahead of .Lfunc_end)
                dcur = desc.setdefault(s.split()[1], [])
            elif s == ".end_amdhsa_kernel":
                dcur = None
            elif dcur is not None:
                dcur.append(s)
            elif cur is not None and s.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
            elif cur is not None:
                cur.append(s)
    return {k: "\n".join(v + ["--"] + desc.get(k, [])) for k, v in out.items() if k in desc}


CLASSES = ("VALU", "SALU", "branch", "wait/nop", "SMEM", "VMEM", "LDS")


def classify(text):
    n = dict.fromkeys(CLASSES, 0)
    vgpr = 0
    body, _, desc = text.partition("\n--\n")
    for s in body.split("\n"):
        op = s.split()[0] if s.split() else ""
        if not op or op.endswith(":") or op.startswith("."):
            continue
        if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc", "s_call")):
            n["branch"] += 1
        elif op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_setprio", "s_sethalt")):
            n["wait/nop"] += 1
        elif op.startswith(("s_load", "s_buffer_load", "s_memrealtime", "s_memtime", "s_dcache_inv")):
            n["SMEM"] += 1
        elif op.startswith("s_"):
            n["SALU"] += 1
        elif op.startswith("ds_"):
            n["LDS"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            n["VMEM"] += 1
        elif op.startswith("v_"):
            n["VALU"] += 1
        else:
            n["SALU"] += 1
    m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc)
    if m:
        vgpr = int(m.group(1))
    return n, vgpr


def demangle(names):
    import shutil
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not tool:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD", help="the commit to compare this tree with")
    ap.add_argument("--jobs", type=int, default=min(32, os.cpu_count() or 1))
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "phase_spec_isa.txt"))
    a = ap.parse_args()
    b = build_module()
    flags = [*b.FLAGS, *b.PRELOAD]
    hipcc = b._hipcc()
    rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", a.parent], text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", a.parent, "kissmcmc.jl_amd/csrc", "include"])
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "parent"))
        trees = {"parent": os.path.join(tmp, "parent", "kissmcmc.jl_amd", "csrc"), "head": os.path.join(PKG, "csrc")}
        jobs = []
        units = {}
        for side, d in trees.items():
            for src in sorted(glob.glob(os.path.join(d, "kmc_inst_*.hip"))):
                u = os.path.basename(src)
                units.setdefault(u, {})[side] = os.path.join(tmp, side + "_" + u + ".s")
                jobs.append((src, units[u][side]))
        with ThreadPoolExecutor(max_workers=a.jobs) as ex:
            list(ex.map(lambda j: compile_asm(hipcc, flags, *j), jobs))
        lines = ["Phase-specialised half-step instance (kmc_kernels.hpp: Spec::Credit): what the change did to the gfx950 code of every kernel instantiation unit.",
                 "`hipcc -S --cuda-device-only` with the build's flags (" + " ".join(flags) + "), this tree (head) against commit " + rev + " (parent);",
                 "comment, .loc, .file and .ident lines, trailing comments and the per-unit __hip_cuid_* symbol left out, block labels renumbered; a kernel's text is its",
                 "body and its kernel descriptor.  Generated by scripts/phase_spec_isa.py.", ""]
        new = {}
        total_same = total_diff = 0
        for u in sorted(units):
            k = {side: kernels_of(p) for side, p in units[u].items()}
            if "parent" not in k:
                new[u] = k["head"]
                continue
            if "head" not in k:
                lines.append(f"{u}: removed ({len(k['parent'])} kernels)")
                continue
            both = sorted(set(k["parent"]) & set(k["head"]))
            diff = [n for n in both if k["parent"][n] != k["head"][n]]
            only_p, only_h = sorted(set(k["parent"]) - set(k["head"])), sorted(set(k["head"]) - set(k["parent"]))
            digest = hashlib.sha256("\n".join(n + "\n" + k["head"][n] for n in both).encode()).hexdigest()[:16]
            total_same += len(both) - len(diff)
            total_diff += len(diff)
            lines.append(f"{u}: {len(both)} kernels in both trees, {len(both) - len(diff)} identical, {len(diff)} differ, {len(only_p)} only in the parent, {len(only_h)} only in head  (sha256 of head's {digest})")
            dm = demangle(diff + only_p + only_h)
            for n in diff:
                lines.append("  differs: " + dm[n])
            for n in only_p:
                lines.append("  only in the parent: " + dm[n])
            for n in only_h:
                lines.append("  only in head: " + dm[n])
        lines += ["", f"existing kernels: {total_same} identical, {total_diff} differ", ""]
        lines.append("New units: static instruction counts (total = " + " + ".join(CLASSES) + ") and VGPRs; `generic` is half_step_vec of the same geometry in kmc_inst_<density>.hip")
        for u in sorted(new):
            base = kernels_of(units[u.replace("_spec", "")]["head"]) if u.replace("_spec", "") in units else {}
            dmb = demangle(sorted(base))
            generic = {}
            for n, t in dmb.items():
                m = re.match(r"void kmc::half_step_vec<kmc::\w+, (\d+), (\d+), (\d+), false, false, double>", t)
                if m:
                    generic[tuple(int(v) for v in m.groups())] = n
            lines.append(f"{u}: {len(new[u])} kernels")
            dm = demangle(sorted(new[u]))
            rows = []
            for n in sorted(new[u]):
                m = re.search(r"<kmc::\w+, (\d+), (\d+), (\d+), \(kmc::Spec\)(\d)>", dm[n])
                geo, sp = (tuple(int(v) for v in m.groups()[:3]), int(m.group(4))) if m else ((0, 0, 0), 0)
                rows.append((geo, sp, n))
            seen = set()
            for geo, sp, n in sorted(rows):
                if geo not in seen and geo in generic:
                    seen.add(geo)
                    c, v = classify(base[generic[geo]])
                    lines.append(f"  L={geo[0]:<2} K={geo[1]} ITER={geo[2]} generic  total {sum(c.values()):4d}  " + "  ".join(f"{x} {c[x]:3d}" for x in CLASSES) + f"  VGPRs {v}")
                c, v = classify(new[u][n])
                lines.append(f"  L={geo[0]:<2} K={geo[1]} ITER={geo[2]} {('generic', 'credit ')[sp]}  total {sum(c.values()):4d}  " + "  ".join(f"{x} {c[x]:3d}" for x in CLASSES) + f"  VGPRs {v}")
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
