"""Every record sink over one small genome that drives each branch of their shared input (SinkInput, vsc_sink.h) and of the
walk over its tiles (the walking kernels of vsc_kernels.hip): a region of reads that spans several tiles, an output region
without any record, regions of one short tile each that one workgroup crosses, and a last region of fewer than 64 reads - all
against the oracle."""
import pytest

import varscot_amd as va
from sink_walk_case import every_sink_equals_the_oracle, sink_walk_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = va.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(oracle):
    """The genome, the oracle's hits with their scores and the oracle forest's votes (sink_walk_case.py: computed once, never changed)."""
    return sink_walk_case(oracle)


@pytest.mark.parametrize("algorithm", ["scan", "seed"])
def test_every_sink_equals_the_oracle(ctx, case, algorithm):
    gen = ctx.load_genome(case["packed"])
    try:
        every_sink_equals_the_oracle(ctx, gen, case, algorithm)
    finally:
        gen.close()
