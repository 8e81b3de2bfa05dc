"""Writes tests/golden/workspace_patch_hunks.json: for every hunk of rust/grayscott_compute_hip.patch, the sha256 of
the lines of the reference checkout that the hunk covers (its old-side range, each line with its newline), keyed by
file and "start,count".  Only hashes are stored, no text of the reference.  tests/test_rust_shim.py hashes the
context and removed lines the patch records for each hunk and compares them with these values: the patch applies
to the reference exactly as long as they agree.
Re-run with a checkout of the reference:  python tests/golden/make_patch_hunks.py REFERENCE_DIR
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATCH = os.path.join(HERE, os.pardir, os.pardir, "rust", "grayscott_compute_hip.patch")


def main(reference: str) -> None:
    out, cur = {}, None
    for raw in open(PATCH).read().splitlines():
        m = re.match(r"^\+\+\+ b/(\S+)", raw)
        if m:
            cur = m.group(1)
            lines = open(os.path.join(reference, cur)).read().splitlines()
            out[cur] = {}
            continue
        m = re.match(r"^@@ -(\d+),(\d+) \+\d+,\d+ @@", raw)
        if m:
            start, count = int(m.group(1)), int(m.group(2))
            assert start + count - 1 <= len(lines), (cur, start, count)
            text = "".join(ln + "\n" for ln in lines[start - 1:start - 1 + count])
            out[cur]["%d,%d" % (start, count)] = hashlib.sha256(text.encode()).hexdigest()
    with open(os.path.join(HERE, "workspace_patch_hunks.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
