"""Developer tool: compare one kernel in two `hipcc --cuda-device-only -S` listings up to register numbering.

    python tools/listing_diff.py parent.s new.s <mangled kernel name> [--show]

Registers, branch labels, literal constants, offsets and the operands of s_waitcnt are masked, directives and comments dropped; what is
left is the instruction stream.  Prints the two instruction counts and how many lines a diff of the two streams touches (0: the same
code up to register allocation and kernel-argument offsets); --show lists the differing groups.  Reads files only."""
import difflib
import re
import sys


def stream(path, kernel):
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
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue
        line = re.sub(r"\b[vsa]\[\d+:\d+\]", "R", line)
        line = re.sub(r"\b[vsa]\d+\b", "R", line)
        line = re.sub(r"\.LBB\d+_\d+", "L", line)
        line = re.sub(r"0x[0-9a-f]+", "K", line)
        line = re.sub(r"offset:\d+", "off", line)
        out.append(re.sub(r"s_waitcnt.*", "s_waitcnt", line))
    return out


def main():
    a, b = stream(sys.argv[1], sys.argv[3]), stream(sys.argv[2], sys.argv[3])
    ops = [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]
    print(len(a), len(b), "instructions; differing lines:", sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops))
    if "--show" in sys.argv:
        for tag, i1, i2, j1, j2 in ops:
            print(tag, i1, a[i1:i2], "->", b[j1:j2])


if __name__ == "__main__":
    main()
