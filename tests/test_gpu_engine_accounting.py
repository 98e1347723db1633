"""What the engine's timers report (-m gpu): launches, flops and bytes per kernel class of every entry point, against
tests/golden/engine_accounting.json.  bench.py's roofline is built from mae_engine_timer_read, so a change of the launch
sequences or of a traffic formula must show up here.  The fixture was generated (tests/golden/make_engine_accounting.py) by
the commit before engine.hip's launch helpers were refactored; equality is exact because every value is a sum of integers
far below 2^53.  Milliseconds are never looked at."""
import json

import pytest

from tests.golden import make_engine_accounting as A

pytestmark = pytest.mark.gpu

GOLD = json.loads(A.FIXTURE.read_text())


def test_fixture_covers_exactly_the_cases():
    assert sorted(GOLD) == sorted(A.CASES)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_timers_report_the_pinned_launches_flops_and_bytes(dev, name):
    got, _outputs = A.run_case(name, dev)
    want = GOLD[name]
    assert sorted(got) == sorted(want), "timer classes differ"
    diff = {cls: (got[cls], want[cls]) for cls in want if got[cls] != want[cls]}
    assert not diff, f"{name}: (got, pinned) {diff}"
    assert sum(t["launches"] for t in got.values()) > 0, "the case timed nothing"
