"""Developer tool: instruction counts by class for one kernel in one or two `hipcc --cuda-device-only -S` listings.

    python tools/listing_classes.py a.s [b.s] <mangled kernel name> [--stretch N]

Prints, per listing, the totals (VALU / SALU / memory) and the classes that tell arithmetic of the step from what merely feeds it:
packed fp32, scalar fp32 arithmetic, plain and wide moves, selects, s_nop, waits, exec-mask SALU (saveexec, branches on exec, SALU
writes of exec), lane spill moves (v_writelane / v_readlane), LDS, global and private memory.  --stretch N adds the same counts for
every stretch of N instructions (where in the kernel a class sits).  The companion of listing_diff.py; reads files only."""
import collections
import re
import sys

CLASSES = (
    ("packed fp32", lambda op, ln: re.fullmatch(r"v_pk_(fma|add|mul)_f32", op)),
    ("  v_pk_fma_f32", lambda op, ln: op == "v_pk_fma_f32"),
    ("  v_pk_add_f32", lambda op, ln: op == "v_pk_add_f32"),
    ("  v_pk_mul_f32", lambda op, ln: op == "v_pk_mul_f32"),
    ("fp32 fma (v_fma + v_fmac)", lambda op, ln: re.fullmatch(r"v_fma(c)?_f32(_e32|_e64|_dpp)?", op)),
    ("fp32 mul", lambda op, ln: re.fullmatch(r"v_mul_f32(_e32|_e64|_dpp)?", op)),
    ("fp32 add + sub", lambda op, ln: re.fullmatch(r"v_(add|sub|subrev)_f32(_e32|_e64|_dpp)?", op)),
    ("plain moves (v_mov_b32)", lambda op, ln: re.fullmatch(r"v_mov_b32(_e32|_e64)?", op)),
    ("wide moves (v_mov_b64 + v_pk_mov_b32)", lambda op, ln: op in ("v_mov_b64", "v_pk_mov_b32")),
    ("selects (v_cndmask)", lambda op, ln: op.startswith("v_cndmask_b32")),
    ("s_nop", lambda op, ln: op == "s_nop"),
    ("waits (s_waitcnt)", lambda op, ln: op.startswith("s_waitcnt")),
    ("exec-mask SALU", lambda op, ln: "saveexec" in op or op.startswith("s_cbranch_exec") or bool(re.match(r"s_\w+\s+exec\b", ln))),
    ("  s_and_saveexec", lambda op, ln: op.startswith("s_and_saveexec")),
    ("  s_cbranch_execz", lambda op, ln: op == "s_cbranch_execz"),
    ("  s_or_b64 (all)", lambda op, ln: op == "s_or_b64"),
    ("lane spill moves (v_writelane + v_readlane)", lambda op, ln: op in ("v_writelane_b32", "v_readlane_b32")),
    ("LDS (ds_)", lambda op, ln: op.startswith("ds_")),
    ("global memory (global_)", lambda op, ln: op.startswith("global_")),
    ("private memory (scratch_ / buffer_)", lambda op, ln: op.startswith("scratch_") or op.startswith("buffer_")),
)


def instructions(path, kernel):
    out, on = [], False
    for line in open(path):
        if line.startswith(kernel + ":"):
            on = True
            continue
        if on and line.startswith(".Lfunc_end"):
            break
        if not on:
            continue
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        out.append(line)
    return out


def counts(lines):
    c = collections.OrderedDict()
    ops = [ln.split()[0] for ln in lines]
    mem = sum(o.startswith(("ds_", "global_", "scratch_", "buffer_", "flat_", "s_load", "s_buffer_load")) for o in ops)
    c["instructions"] = len(ops)
    c["VALU"] = sum(o.startswith("v_") for o in ops)
    c["SALU"] = sum(o.startswith("s_") and not o.startswith(("s_load", "s_buffer_load")) for o in ops)
    c["memory"] = mem
    for name, test in CLASSES:
        c[name] = sum(bool(test(o, ln)) for o, ln in zip(ops, lines))
    return c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    stretch = int(sys.argv[sys.argv.index("--stretch") + 1]) if "--stretch" in sys.argv else 0
    if stretch:
        args = args[:-1]
    *paths, kernel = args
    streams = [instructions(p, kernel) for p in paths]
    if not all(streams):
        sys.exit(f"{kernel}: not found in every listing")
    cols = [counts(s) for s in streams]
    print(f"{'':46s}" + "".join(f"{p[-22:]:>24s}" for p in paths))
    for k in cols[0]:
        print(f"{k:46s}" + "".join(f"{c[k]:24d}" for c in cols))
    if stretch:
        for p, s in zip(paths, streams):
            print(f"\n{p}: per stretch of {stretch} instructions: packed / plain moves / selects / s_nop / exec-mask / lane spill / LDS / private")
            for i in range(0, len(s), stretch):
                c = counts(s[i:i + stretch])
                print(f"{i:6d}  " + " ".join(f"{c[k]:5d}" for k in ("packed fp32", "plain moves (v_mov_b32)", "selects (v_cndmask)", "s_nop", "exec-mask SALU",
                                                                      "lane spill moves (v_writelane + v_readlane)", "LDS (ds_)",
                                                                      "private memory (scratch_ / buffer_)")))


if __name__ == "__main__":
    main()
