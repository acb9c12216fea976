"""The rollout kernel instantiations in the build are exactly those a launch can reach (no GPU, nothing is launched): the
`rollout_*_kernel` functions of the built objects, read as tools/kernel_metadata.py reads them, equal the list
profiles/rollout_kernels_reachable.txt -- what tools/reachable_rollout_kernels.py found reachable through the entry points, plus the
file's short "kept" section -- and hold every kernel tests/golden/rollout_routes_gpu.json names.  An instantiation no route reaches
cannot be tested or measured: adding one fails here, and so does dropping one a route needs."""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
LIST = os.path.join(REPO, 'profiles', 'rollout_kernels_reachable.txt')
ROUTES = os.path.join(REPO, 'tests', 'golden', 'rollout_routes_gpu.json')
_KERNEL = re.compile(r'mf::rollout_\w+_kernel<[^()<>]*>')


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as g
    from kernel_metadata import kernels
    g.build()
    return {n for _, n, _ in kernels() if _KERNEL.fullmatch(n)}


def listed():
    """(reachable, kept) names of the profile file: one per line, `#` starts a comment, the kept section follows its `##` heading."""
    from reachable_rollout_kernels import KEPT
    parts = {False: set(), True: set()}
    kept = False
    for line in open(LIST):
        kept = kept or line.startswith(KEPT)
        name = line.split('#')[0].strip()
        if name:
            assert _KERNEL.fullmatch(name), line
            parts[kept].add(name)
    return parts[False], parts[True]


def test_the_build_holds_the_reachable_kernels_and_no_others(built):
    reachable, kept = listed()
    assert len(reachable) > 800 and not (reachable & kept)
    assert sorted(built - reachable - kept) == [], 'instantiated, but no launch reaches them (tools/reachable_rollout_kernels.py)'
    assert sorted((reachable | kept) - built) == [], 'a launch can reach them (or the list keeps them), but they are not built'


def test_every_recorded_route_names_a_built_kernel(built):
    named = set(_KERNEL.findall(json.dumps(json.load(open(ROUTES)))))
    assert len(named) > 60
    assert sorted(named - built) == []
