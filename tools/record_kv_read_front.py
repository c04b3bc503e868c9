#!/usr/bin/env python3
"""Record what the Python front of the sixteen KV-cache reading calls does on the corpus of tests/kv_read_front_cases.py, as
JSON: for every accepted call the bindings reached and their arguments, for every refused one the exception's type and message.

Run it on a checkout of the commit whose behaviour is to be kept (a built one: the refusals are recorded on the real extension)
and commit the output as tests/golden/kv_read_front.json; tests/test_kv_read_front_host.py replays the corpus against it.

    python tools/record_kv_read_front.py --commit "$(git rev-parse HEAD)" > kv_read_front.json
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "matrix-multiplication_amd", REPO / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import kv_read_front_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit the recording is made on (kept in the file)")
    args = ap.parse_args()
    accepted, refused = cases.replay()
    silent = [f"{call}: {case}" for call, of_call in refused.items() for case, (kind, *_) in of_call.items() if kind == "no exception"]
    if silent:
        sys.exit("a refusal was intended but nothing was raised — a mistake in the corpus:\n  " + "\n  ".join(silent))
    strings = {}
    packed = {"accepted": cases.pack(accepted, strings), "refused": cases.pack(refused, strings)}
    json.dump({"recorded_on": args.commit, "strings": list(strings), **packed}, sys.stdout, separators=(",", ":"), ensure_ascii=False)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
