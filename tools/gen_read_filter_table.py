#!/usr/bin/env python3
"""The literals of csrc/vgmi_read_filter.h's error table, by exact decimal arithmetic:

    E10[t] = round_half_even(10^(-t/100) * 2^30)      t = 0 .. 930

10^(-t/100) is computed with 80 significant digits where the result has 10, far more than the distance of any entry from a half.
Prints the rows as they stand in the header; `--check HEADER` compares them with the header's.
"""
import re
import sys
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

N = 931


def table():
    getcontext().prec = 80
    out = []
    for t in range(N):
        x = (Decimal(10) ** (Decimal(-t) / Decimal(100))) * Decimal(2 ** 30)
        out.append(int(x.quantize(Decimal(1), rounding=ROUND_HALF_EVEN)))
    return out


def rows(values, per=10):
    lines = []
    for i in range(0, len(values), per):
        lines.append("        " + " ".join("%du," % v for v in values[i:i + per]) + "      // %d" % i)
    return "\n".join(lines)


def header_values(path):
    text = open(path).read()
    body = text[text.index("VGH_E10_BEGIN"):text.index("VGH_E10_END")]
    body = re.sub(r"//[^\n]*", "", body)
    return [int(m) for m in re.findall(r"\b(\d+)u,", body)]


def main():
    v = table()
    if len(sys.argv) == 3 and sys.argv[1] == "--check":
        h = header_values(sys.argv[2])
        if h != v:
            sys.exit("the header's table differs from the computed one")
        print("ok: %d entries" % len(h))
        return
    print(rows(v))


if __name__ == "__main__":
    main()
