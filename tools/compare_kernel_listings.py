#!/usr/bin/env python
"""Compare two `hipcc -S --cuda-device-only` listings of one kernel file kernel by kernel: are the instruction streams the
same?  Labels, symbol names, comments and section directives are normalised away, and kernels are matched by their plain
name and integer template argument, so a kernel that became a template over its element type (`vae_conv_kernel<9>` ->
`vae_conv_kernel<9, half_t>`, `unet_gn_lds_kernel` -> `unet_gn_lds_kernel_t<half_t>`) is compared with what it was.
DESIGN.md section 19.1 records such a comparison.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -S --cuda-device-only fresco_amd/csrc/vae.hip -o after.s
    python tools/compare_kernel_listings.py before.s after.s       # exit status 1 if any kernel differs or is missing
"""
import re
import sys


def kernels(path):
    """{mangled name: normalised instruction lines} of every function of the listing"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\.Lfunc_end\d+:", open(path).read(), re.S | re.M):
        body = re.sub(r";.*", "", re.sub(r"_Z\w+", "SYM", re.sub(r"\.L\w+", "L", m.group(2))))
        out[m.group(1)] = [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((".section", ".text"))]
    return out


def key(name):
    plain = re.search(r"_ZN\d+\w*?\d+([a-z_0-9]*?_kernel)(?:_t)?I?", name)
    arg = re.search(r"ILi(\d+)E", name)
    return (plain.group(1) if plain else name) + ("<%s>" % arg.group(1) if arg else "")


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    ka, kb = {key(n): n for n in a}, {key(n): n for n in b}
    bad = 0
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            print("%-40s only in %s" % (k, sys.argv[1] if k in ka else sys.argv[2]))
            bad += 1
            continue
        x, y = a[ka[k]], b[kb[k]]
        same = x == y
        bad += not same
        print("%-40s %6d lines  %s" % (k, len(x), "identical" if same else "DIFFERENT (%d lines after)" % len(y)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
