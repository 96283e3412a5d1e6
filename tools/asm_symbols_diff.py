"""Compare the device code of every kernel between two `hipcc --cuda-device-only -S` listings of the same source file.

    python tools/asm_symbols_diff.py before.s after.s

Prints the symbols whose instruction text differs, the symbols only one side has, and exits 1 when a common symbol differs.  Local
labels carry the function's ordinal (.LBB12_3), which shifts when a kernel is added in front: they are compared without it."""
import re
import sys


def bodies(path):
    out, name, buf = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, buf = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = buf
                name = None
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip())
            if line:
                buf.append(line)
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print(f"{len(a)} / {len(b)} symbols; common {len(set(a) & set(b))}; identical {len(set(a) & set(b)) - len(differ)}")
    for k in differ:
        print("DIFFERS", k, len(a[k]), len(b[k]))
    for k in sorted(set(a) - set(b)):
        print("ONLY BEFORE", k)
    for k in sorted(set(b) - set(a)):
        print("ONLY AFTER", k, len(b[k]), "lines")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
