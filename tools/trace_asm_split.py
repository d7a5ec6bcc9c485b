"""Static instruction split of k_trace (no GPU): compiles rt_render.hip (the render kernels' unit) to gfx950 assembly with line
tables, attributes every instruction of one kernel to the source function its line lies in (the
innermost inlined frame the compiler recorded) and sums the functions into the parts of a query's
life: setup, refill/begin, visit, walk-end (verify, store) and drain. A helper that many callers share
(dot, rt_max, a ballot) and compiler-generated code without a line count with the part around them.

  python tools/trace_asm_split.py [--kernel SUBSTR] [--json OUT] [--functions] [--csrc DIR] [-- extra hipcc flags]

The visit is split further into the pieces of a trip ("visit_parts"): box test, ranking, push, pop,
leaf and loop control (quad_visit's own loop and returns, and trace_stream's trip loop around it), by
marker strings in quad_visit (VISIT_MARKS; --csrc DIR splits another checkout's csrc/ with the same
markers). A marker that is not found in quad_visit is reported on stderr: the pieces after it are
then counted with the piece before.

The counts are static (instructions in the code object, each once), not executed counts: they say
how long each region is for a wave that enters it, which is what a divergent region costs however
few quads are in it. Spill traffic (scratch_load / scratch_store) is listed per part.

The split is approximate. A line table names one source line per instruction, after the
scheduler has mixed neighbouring regions; the parts are found by function names and by marker
strings in trace_stream (function_map below), so an edit there can move instructions between
parts: compare two builds only with the same markers in place, and read differences of a few
per cent as noise.
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

from kernel_regs import HIPCC, HIPCC_FLAGS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sycl-ray-tracing_amd", "csrc")
FLAGS = [*HIPCC_FLAGS, "--cuda-device-only", "-gline-tables-only", "-S"]

# source function -> part of a query's life
PARTS = {
    "begin": {"qstate_begin", "rayb_setup", "forced_fallback", "far_origin", "queue_item_ptr", "qbase", "queue_prefetch",
              "trace_stream:refill", "v3of"},
    "visit": {"quad_visit", "quad_child", "child_record", "box_hit2", "box_hit", "slab_ok", "rt_half", "quad_tri",
              "tri_test_v", "tri_test", "leaf_item", "qdpp", "qdppf", "qor", "qsum", "s_lower", "rec", "key", "set",
              "set_rec", "fuzzy_tri", "trace_stream:loop", "QuadStack"},
    "verify": {"quad_chain_ok", "quad_chain_ray", "chain_lane", "slab_div", "quad_closest_answer", "normal"},
    "store": {"trace_stream:finish", "finish_any", "finish_closest", "walk_log", "spheres_closest",
              "sphere_test"},
    "setup": {"shard_prefix", "shard_find8", "split_blocks", "seg_id", "seg_counter", "qc_at", "hc_at", "ac_at",
              "__launch_bounds__", "k_trace", "flush_stats", "trace_stream:setup"},
    "drain": {"trace_stream:drain", "row_visit", "row_min", "row_minf", "row_or", "row_rank_from", "row_rank",
              "row_bits", "rdpp", "rdppf", "RowInQuadStack"},
}
FUNC_PART = {f: p for p, fs in PARTS.items() for f in fs}
# the visit's pieces: helper functions by name, quad_visit's own lines by marker (VISIT_MARKS, in source order)
VISIT_SUB = {
    "box": {"quad_child", "child_record", "box_hit2", "box_hit", "slab_ok", "rt_half", "leaf_item", "quad_visit:box"},
    "rank": {"s_lower", "quad_visit:rank"},
    "push": {"set", "set_rec", "quad_visit:push"},
    "pop": {"pop_within", "rec", "key", "quad_visit:pop"},
    "leaf": {"quad_tri", "tri_test_v", "tri_test", "fuzzy_tri", "quad_visit:leaf"},
    "loopctl": {"trace_stream:loop", "quad_visit:loopctl", "cur_inner"},
}
FUNC_SUB = {f: p for p, fs in VISIT_SUB.items() for f in fs}
VISIT_MARKS = [("for (int dd = 0;", "loopctl"), ("int nd[NW];", "pop"), ("float4_ r0[NW], r1[NW];", "box"),
               ("const int o = ok ? 1 : 0;", "rank"), ("stack position sp + k - 1", "push"),
               ("st->c[RT_STAT_VOL] += 4;", "box"), ("rank by (key, lane)", "rank"), ("const int nv = qsum(", "push"),
               ("// (descended DESC times; still inner)", "loopctl"), ("if (q.cur < 0) {", "leaf"),
               ("// (h.k = 0: no occluder)", "pop")]
DEF = re.compile(r"^(?!\s|#|//|namespace|struct|class|template|using|typedef|static_assert|\}|\{)[^;]*?\b([A-Za-z_]\w*)\s*\(")


def function_map(path):
    """line number -> enclosing function (column-0 definitions; trace_stream split into its phases)."""
    out, cur, phase, seen = {}, None, None, set()
    with open(path, errors="replace") as f:
        for n, line in enumerate(f, 1):
            m = DEF.match(line) or re.match(r"^struct\s+(\w+)[^;]*$", line)  # (a struct's members count with it)
            if m and not line.rstrip().endswith(";"):
                cur, phase = m.group(1), None
            if cur == "quad_visit":
                for mark, ph in VISIT_MARKS:
                    if mark in line:
                        phase = ph
                        seen.add(mark)
                out[n] = "quad_visit:" + (phase or "loopctl")
            elif cur == "trace_stream":
                if "auto finish = [&]" in line:
                    phase = "finish"
                elif phase == "finish" and line.startswith("    };"):
                    out[n] = "trace_stream:finish"
                    phase = "loop"
                    continue
                elif "const unsigned long long bidle" in line:
                    phase = "refill"
                elif "const unsigned long long bact = __ballot" in line and phase == "refill":
                    phase = "loop"
                elif "The drain as rows" in line:
                    phase = "drain"
                out[n] = "trace_stream:" + (phase or "setup")
            else:
                out[n] = cur
    if "quad_visit" in out.values() or any(str(v).startswith("quad_visit:") for v in out.values()):
        for mark, ph in VISIT_MARKS:
            if mark not in seen:
                print(f"trace_asm_split: marker {mark!r} ({ph}) not found in quad_visit of {path}", file=sys.stderr)
    return out


def split(kernel, extra, csrc=CSRC):
    src = os.path.join(csrc, "rt_render.hip")
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        subprocess.run([HIPCC, *FLAGS, *extra, src, "-o", asm], check=True, stderr=subprocess.DEVNULL)
        lines = open(asm, errors="replace").read().splitlines()
    files, maps = {}, {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            p = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
            files[int(m.group(1))] = p
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(kernel) + r"\w*:", l))
    name = lines[start].split(":")[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    cnt = collections.Counter()
    parts = collections.Counter()
    spill = collections.Counter()
    kinds = collections.defaultdict(collections.Counter)
    func, part, sub = "?", "setup", "loopctl"  # (helpers such as dot or rt_max, and line-0 code, count with the part around them)
    vparts = collections.Counter()
    vkinds = collections.defaultdict(collections.Counter)
    for l in lines[start + 1:end]:
        s = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            path = files.get(int(m.group(1)), "")
            if os.path.isfile(path) and path not in maps:
                maps[path] = function_map(path)
            func = maps.get(path, {}).get(int(m.group(2))) or os.path.basename(path) + ":?"
            part = FUNC_PART.get(func.split(":")[0] if func.startswith("quad_visit:") else func, part)
            sub = FUNC_SUB.get(func, sub)
            continue
        if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        cnt[func] += 1
        parts[part] += 1
        kind = "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "mem"
        kinds[part][kind] += 1
        if part == "visit":
            vparts[sub] += 1
            vkinds[sub]["branch" if op.startswith(("s_cbranch", "s_branch")) else kind] += 1
        if op.startswith(("scratch_load", "scratch_store")):
            spill[part + (":load" if "load" in op else ":store")] += 1
    return {"kernel": name, "instructions": sum(cnt.values()), "parts": dict(parts),
            "kinds": {p: dict(k) for p, k in kinds.items()}, "spill_ops": dict(spill),
            "visit_parts": dict(vparts), "visit_kinds": {p: dict(k) for p, k in vkinds.items()},
            "functions": dict(cnt.most_common())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="k_traceILb0ELb1ELi4ELi0E")
    ap.add_argument("--json")
    ap.add_argument("--functions", action="store_true")
    ap.add_argument("--csrc", default=CSRC, help="the csrc/ directory to compile (default: this checkout's)")
    args, rest = ap.parse_known_args()
    r = split(args.kernel, [a for a in rest if a != "--"], args.csrc)
    print(r["kernel"], "instructions", r["instructions"])
    for p, n in sorted(r["parts"].items(), key=lambda x: -x[1]):
        print(f"  {p:8s} {n:6d}  {100.0 * n / r['instructions']:5.1f} %  {r['kinds'][p]}")
    for p, n in sorted(r["visit_parts"].items(), key=lambda x: -x[1]):
        print(f"    visit/{p:8s} {n:6d}  {100.0 * n / r['instructions']:5.1f} %  {r['visit_kinds'][p]}")
    print("  spill ops", r["spill_ops"])
    if args.functions:
        for f, n in r["functions"].items():
            print(f"    {f:32s} {n}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(r, f, indent=1)
