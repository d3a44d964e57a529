"""Compare the gfx950 instructions of kernels in two builds of a unit, register names aside.

    python scripts/isa_diff.py OLD.o NEW.o [KERNEL_SUBSTRING ...]

OLD.o / NEW.o are `hipcc -c` objects of the same unit (for example rpe_volume.o of the parent commit and of this tree).  Every kernel
whose mangled name contains one of the substrings (all kernels when none is given) is disassembled from both; each instruction is
reduced to its text with v/s/a registers, register ranges and branch labels replaced by placeholders and addresses dropped; so is the
pc-relative literal of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 (the distance to a constant table, which moves when
anything in the unit changes size).  Prints one line per kernel, "same" or the first differing instruction, and exits 1 if any kernel differs or is missing from either side."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa_tools as T  # noqa: E402

REG = re.compile(r"\b([vsa])(\d+|\[\d+:\d+\])")
LABEL = re.compile(r"\bL\d+\b")
LITERAL = re.compile(r",\s*(0x[0-9a-f]+|-?\d+)$")


def normalise(body):
    out, pc = [], 0   # pc: how many of the two adds behind an s_getpc_b64 are still to come
    for i in body:
        t = i.text
        if t.startswith("s_getpc_b64"):
            pc = 2
        elif pc and t.startswith(("s_add_u32", "s_addc_u32")):
            t, pc = LITERAL.sub(", pcrel", t), pc - 1
        else:
            pc = 0   # only the pair directly behind the s_getpc_b64
        out.append(LABEL.sub("L", REG.sub(lambda m: m.group(1) + "#", t)))
    return out


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    old, new = T.disassemble(argv[0]), T.disassemble(argv[1])
    keys = argv[2:]
    names = sorted(n for n in set(old) | set(new) if not keys or any(k in n for k in keys))
    bad = 0
    for n in names:
        if n not in old or n not in new:
            print(f"{n}: only in {'new' if n in new else 'old'}")
            bad += 1
            continue
        a, b = normalise(old[n]), normalise(new[n])
        if a == b:
            print(f"{n}: same ({len(a)} instructions)")
            continue
        bad += 1
        k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"{n}: differs at instruction {k} of {len(a)} / {len(b)}: {a[k] if k < len(a) else '-'} | {b[k] if k < len(b) else '-'}")
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
