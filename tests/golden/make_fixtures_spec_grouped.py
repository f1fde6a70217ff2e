#!/usr/bin/env python3
"""What tests/test_spec_graph_cpu.py pins the case lists of spec_graph_cases.py against, around the grouped lists:

    python tests/golden/make_fixtures_spec_grouped.py digests TESTS_DIR
    python tests/golden/make_fixtures_spec_grouped.py coverage

digests   TESTS_DIR: the tests/ directory of the commit BEFORE spec_graph_cases.py learnt the gconv op (the commit "Add
          grouped convolution: C ABI, HIP kernels, layers, spec op, importer").  Run against a later tree it records that
          tree's lists, which proves nothing.
            spec_grouped_parent.json   digest (spec_digest.spec_digest) of every HAND and HAND_WIDE case and of
                                       generate(seed) / generate_wide(seed) for every seed of SEEDS / SEEDS_WIDE
coverage  on this tree:
            spec_grouped_coverage.json per category of REQUIRED_GROUPED the first two hand-written cases or unrejected
                                       seeds that cover it, hand-written cases first
No test runs this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MODE = sys.argv[1] if len(sys.argv) > 1 else ""
TESTS = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository: oracle/
sys.path.insert(0, os.path.dirname(HERE))                        # spec_digest.py
sys.path.insert(0, TESTS)

import spec_digest as G                   # noqa: E402
import spec_graph_cases as S              # noqa: E402


def digests():
    lists = {"hand": {c["name"]: G.spec_digest(c["spec"], c["x"]) for c in S.HAND},
             "generated": {str(seed): G.spec_digest(*S.generate(seed)) for seed in S.SEEDS},
             "hand_wide": {c["name"]: G.spec_digest(c["spec"], c["x"]) for c in S.HAND_WIDE},
             "generated_wide": {str(seed): G.spec_digest(*S.generate_wide(seed)[:2]) for seed in S.SEEDS_WIDE}}
    with open(os.path.join(HERE, "spec_grouped_parent.json"), "w") as f:
        json.dump(lists, f, indent=1, sort_keys=True)
    print("recorded %s from %s" % (", ".join("%d %s" % (len(v), k) for k, v in sorted(lists.items())), TESTS))


def coverage():
    cover = {}
    for c in S.HAND_GROUPED:
        for k in S.categories_grouped(c["spec"], c["image"]):
            cover.setdefault(k, []).append(c["name"])
    for seed in S.SEEDS_GROUPED:
        spec, x, image = S.generate_grouped(seed)
        if S.guard(spec, x) is None:
            for k in S.categories_grouped(spec, image):
                cover.setdefault(k, []).append("seed %d" % seed)
    with open(os.path.join(HERE, "spec_grouped_coverage.json"), "w") as f:
        json.dump({k: cover[k][:2] for k in sorted(S.REQUIRED_GROUPED)}, f, indent=1, sort_keys=True)
    print("recorded %d categories" % len(S.REQUIRED_GROUPED))


if __name__ == "__main__":
    {"digests": digests, "coverage": coverage}[MODE]()
