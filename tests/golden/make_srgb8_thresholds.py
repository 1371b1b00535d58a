"""Writes tests/golden/srgb8_thresholds.json: the table T[1..255] of docs/SPEC.md §10 as 255 u32 bit patterns, and prints the same
values as the hex-float literals of pathtracing_amd/csrc/display_table.h (`--header`).

T[k] is the smallest f32 y with floor(255 * oetf(y) + 0.5) >= k, where oetf is the sRGB OETF evaluated in float64. The f32 nearest to
the inverse OETF of (k - 0.5)/255 is a first guess only; it is then stepped to the neighbour the definition asks for."""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def oetf(y):
    y = np.asarray(y, np.float64)
    return np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(np.maximum(y, 0.0), 1.0 / 2.4) - 0.055)


def code64(y):
    """floor(255 * oetf(y) + 0.5) in float64, of f32 values in [0, 1]."""
    return np.floor(255.0 * oetf(np.asarray(y, np.float32).astype(np.float64)) + 0.5).astype(np.int64)


def inverse_oetf(e):
    return e / 12.92 if e <= 12.92 * 0.0031308 else ((e + 0.055) / 1.055) ** 2.4


def thresholds():
    """(T as a float32 array of 256 entries with T[0] = 0, the number of entries the first guess missed)."""
    t = np.zeros(256, np.float32)
    stepped = 0
    for k in range(1, 256):
        y = np.float32(inverse_oetf((k - 0.5) / 255.0))
        y0 = y
        while code64(np.nextafter(y, np.float32(-1.0))) >= k:
            y = np.nextafter(y, np.float32(-1.0))
        while code64(y) < k:
            y = np.nextafter(y, np.float32(2.0))
        stepped += int(y != y0)
        t[k] = y
    return t, stepped


def main():
    t, stepped = thresholds()
    bits = [int(b) for b in t[1:].view(np.uint32)]
    if "--header" in sys.argv:
        vals = [re.sub(r"0+p", "p", float(v).hex()) + "f" for v in t[1:]]
        for i in range(0, 255, 6):
            print("    " + ", ".join(vals[i:i + 6]) + ",")
        return
    with open(os.path.join(HERE, "srgb8_thresholds.json"), "w") as f:
        json.dump({"what": "docs/SPEC.md §10: T[k], k = 1..255, as f32 bit patterns", "first_guess_missed": stepped, "bits": bits}, f)
        f.write("\n")
    print(f"wrote 255 thresholds ({stepped} stepped off the rounded inverse)")


if __name__ == "__main__":
    main()
