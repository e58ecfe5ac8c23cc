"""The launch structure of the four batch RANSAC searches as the profile reports it: what tools/homography_batch_bench.py,
tools/fundamental_time.py, tools/resect_time.py and tools/align_time.py read.  With the profile on, a call reports exactly
its own entries, one call per launch scope, and nothing else; without an entry to search, resect reports its pick alone
and align nothing.  The cases are the smallest the calls' own tests have (used_context.py), the two searches on frames at
65 loops so that two hypothesis blocks exist."""
import pytest

import align_cases as AC
import resect_cases as RS
import used_context as U
from batch_util import guarded_context

pytestmark = pytest.mark.gpu

LOOPS = 65
ENTRIES = dict(
    find_homography_batch=("homo_batch_gather", "homo_batch_solve", "homo_batch_count", "homo_batch_pick"),
    find_fundamental_batch=("fund_batch_gather", "fund_batch_solve", "fund_batch_count", "fund_batch_pick"),
    resect_cameras_batch=("resect_gather", "resect_solve", "resect_count", "resect_pick"),
    align_points_batch=("align_gather", "align_solve", "align_count", "align_pick", "align_refit"))
EMPTY = dict(resect_cameras_batch=("resect_pick",), align_points_batch=())


@pytest.fixture(scope="module")
def g():
    with guarded_context(1) as c:
        yield c


def _cases(name):
    """The step's small case, and for resect and align the same scene without an entry."""
    step = U.step(name)
    case = step.case("small")
    if name == "resect_cameras_batch":
        assert list(case["images"]) == [2, 3, 0]
        assert (case["max_cand"], case["num_loops"], case["min_inliers"]) == (91, 49, 12)
        return step, ((case, ENTRIES[name]), (RS.resect_case(RS.small_scene()["case"], []), EMPTY[name]))
    if name == "align_points_batch":
        assert len(case["ranges"]) == 4
        return step, ((case, ENTRIES[name]), (AC.gpu_cases()["nsel 0"], EMPTY[name]))
    return step, ((dict(case, loops=LOOPS), ENTRIES[name]),)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_profile_entries_and_calls(g, name):
    step, runs = _cases(name)
    for case, want in runs:
        dev = {k: g.upload(v) for k, v in list(step.uploads(case).items()) + list(step.outputs(case).items())}
        lists = step.lists(case)
        g.sync()
        g.profile_enable(True)
        g.profile_reset()
        try:
            step.enqueue(g, case, dev, lists)
            g.sync()
            read = g.profile_read()
        finally:
            g.profile_enable(False)
        got = {k: v["calls"] for k, v in read.items()}
        print(name, got)
        assert got == {k: 1 for k in want}, (name, got)
