#!/usr/bin/env python3
"""Generate tests/golden/converter_keys.json from the reference's checkpoint converter.  TEST INFRASTRUCTURE.

Runs only where the reference tree exists (like gen_golden.py); its OUTPUT is committed, so tests/test_converter_keys.py
needs nothing outside the repository.  The converter (Pai-Megatron-Patch/toolkits/model_checkpoints_convertor/llava/
hf2megatron_llava.py) is parsed, never executed: the fixture holds the tensor-name fragments among its string literals
(literals made only of name characters with at least one '.', f-strings as written) and its q / k / v index map.

usage:  python oracle/gen_converter_keys.py --reference DIR      (rewrites tests/golden/converter_keys.json)
"""
from __future__ import annotations

import argparse
import io
import json
import os
import re
import tokenize

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "converter_keys.json")
CONV = "Pai-Megatron-Patch/toolkits/model_checkpoints_convertor/llava/hf2megatron_llava.py"


def string_literals(src: str) -> set:
    lit = set()
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):          # every string literal of the file, f-strings as written
        if tok.type == tokenize.STRING:
            body = re.sub(r"^[rbfuRBFU]*", "", tok.string)
            q = body[:3] if body[:3] in ('"""', "'''") else body[:1]
            lit.add(body[len(q):-len(q)])
    return lit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (the directory holding Pai-Megatron-Patch/)")
    args = ap.parse_args()
    src = open(os.path.join(args.reference, CONV)).read()
    names = sorted(l for l in string_literals(src) if "." in l and re.fullmatch(r"[\w.{}\[\]]+", l))
    m = re.search(r"QKV = \{0: '(\w+)', 1: '(\w+)', 2: '(\w+)'\}", src)
    out = {"source": CONV, "name_literals": names, "qkv_index_map": list(m.groups()) if m else None}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{OUT}: {len(names)} name literals, qkv map {out['qkv_index_map']}")


if __name__ == "__main__":
    main()
