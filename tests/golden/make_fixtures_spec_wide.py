#!/usr/bin/env python3
"""What tests/test_spec_graph_cpu.py pins the shared reference and the old case lists against:

    python tests/golden/make_fixtures_spec_wide.py [TESTS_DIR]

TESTS_DIR: the tests/ directory of the commit BEFORE spec_graph_cases.py learnt concat, the spatial ops, dwconv and
tconv (the commit "Add Conv2DTranspose: C ABI, HIP kernels, layers, spec op, importer"), where concat_cases.py and
spatial_cases.py still hold their own reference and guard.  Run against a later tree it records that tree's functions,
which proves nothing.  No test runs this file.

  spec_graph_parent.json     digest (spec_digest.spec_digest) of every spec_graph_cases.HAND case and of generate(seed)
                             for every seed in SEEDS
  spec_wide_old_reference.npz, .json
                             concat_cases.reference / guard on concat_cases.SPECS and spatial_cases.reference / guard on
                             spatial_cases.SPECS, CHAINS, binary_pad and binary_upsample: the last tensor as an array,
                             the digest of every tensor of the network, the guard's answer
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository: oracle/
sys.path.insert(0, os.path.dirname(HERE))                        # spec_digest.py
sys.path.insert(0, TESTS)

import spec_digest as G                   # noqa: E402
import concat_cases as C                  # noqa: E402
import spatial_cases as SP                # noqa: E402
import spec_graph_cases as S              # noqa: E402


def old_cases():
    """(name, net, reference, guard) of every spec the two files ran under their own reference."""
    out = [("concat/" + n, net, C.reference, C.guard) for n, (net, _) in C.SPECS.items()]
    out += [("spatial/" + n, net, SP.reference, SP.guard) for n, (net, _) in SP.SPECS.items()]
    out += [("chain/" + n, net, SP.reference, SP.guard) for n, (net, _) in SP.CHAINS.items()]
    out += [("spatial/binary_pad", SP.binary_pad(), SP.reference, SP.guard),
            ("spatial/binary_upsample", SP.binary_upsample(), SP.reference, SP.guard)]
    return out


def main():
    lists = {"hand": {c["name"]: G.spec_digest(c["spec"], c["x"]) for c in S.HAND},
             "generated": {str(seed): G.spec_digest(*S.generate(seed)) for seed in S.SEEDS}}
    with open(os.path.join(HERE, "spec_graph_parent.json"), "w") as f:
        json.dump(lists, f, indent=1, sort_keys=True)
    arrays, meta = {}, {}
    for name, net, reference, guard in old_cases():
        x = net.images()
        env = reference(net.spec, x, return_all=True)
        arrays[name] = env[S.names_of(net.spec)[-1]]
        meta[name] = {"spec": G.spec_digest(net.spec, x), "guard": guard(net.spec, x),
                      "tensors": {k: G.array_digest(v) for k, v in env.items()}}
    np.savez_compressed(os.path.join(HERE, "spec_wide_old_reference.npz"), **arrays)
    with open(os.path.join(HERE, "spec_wide_old_reference.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("recorded %d hand, %d generated, %d old-reference cases from %s"
          % (len(lists["hand"]), len(lists["generated"]), len(meta), TESTS))


if __name__ == "__main__":
    main()
