"""GPU: the launch schedule of every step form -- which C-ABI entries, in which order, on which streams, with which wait edges
and how many record_stream calls per stream -- equals the schedule recorded from the commit before the head's orchestration was
split into phases (tests/head_schedule_ref.py; the last five forms, one per remaining route of cluster_fused.cluster_route, from
the commit before the route plan), and the losses are the same bits.  Losses alone cannot see a branch that is issued late; a
captured graph starts its nodes in the order they were issued."""
import pytest

import head_schedule_ref as REF
import head_trace

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", list(head_trace.FORMS))
def test_schedule_and_losses_equal_the_recorded_ones(form):
    trace, losses = head_trace.run_form(form)
    want = REF.TRACES[form]
    first = next((i for i, (a, b) in enumerate(zip(trace, want)) if a != b), min(len(trace), len(want)))
    print(f"\n[{form}] {len(trace)} entries (recorded: {len(want)}); losses {losses}")
    assert trace == want, f"first difference at entry {first}: got {trace[first:first + 4]}, recorded {want[first:first + 4]}"
    assert losses == REF.LOSSES[form], (losses, REF.LOSSES[form])
