"""What sweeping the bias shows, on the CPU in fp64 (tests/align_ref.py on tests/longmem_ref.py's campaign items): the cells of the
README's failing table -- emerging items, start = 1.0, B = 4 and 8, the three shapes, seeds 0 / 1 / 2 -- as wrong labels per
memory_bias in {0, 0.05, 0.1, 0.2, 0.4}.  SYNTHETIC ONLY: nothing here says anything about MCoRDS or SHARAD.

The test asserts consistency alone: the b = 0 and b = 0.1 columns are the counts the README already quotes (tests/test_longmem.py and
tests/test_align.py re-measure those).  It does not assert that some bias wins; the table is printed for the reader."""
import pytest

import align_ref as ar
import sliding_ref as slr
from test_align import BIASED_START_1, NAMES

BIASES = (0.0, 0.05, 0.1, 0.2, 0.4)
# without the bias (tests/test_align.py's comment, tests/test_longmem.py's table): B -> shape -> seeds 0 / 1 / 2
UNBIASED_START_1 = {4: ((143, 0, 0), (0, 0, 0), (893, 898, 898)), 8: ((143, 0, 0), (0, 0, 0), (843, 898, 898))}


@pytest.fixture(scope="module")
def table():
    """{(B, shape index, bias): wrong labels of seeds 0 / 1 / 2}"""
    t = {(B, k, b): tuple(ar.aligned_errors(slr.DRIFT_SHAPES[k], s, B, 1.0, True, bias=b)[0] for s in range(3))
         for B in (4, 8) for k in range(3) for b in BIASES}
    print("SYNTHETIC ONLY -- emerging items at start 1.0, wrong labels among the frames >= T // 3, seeds 0 / 1 / 2, per memory_bias:")
    print("    {:>2} {:>10} ".format("B", "shape") + " ".join("{:>17}".format(f"b = {b:g}") for b in BIASES))
    for B in (4, 8):
        for k in range(3):
            print("    {:>2} {:>10} ".format(B, NAMES[k]) + " ".join("{:>17}".format(" / ".join(map(str, t[(B, k, b)]))) for b in BIASES))
    return t


def test_the_columns_the_readme_quotes_are_what_they_were(table):
    for B in (4, 8):
        assert tuple(table[(B, k, 0.0)] for k in range(3)) == UNBIASED_START_1[B], B
        assert tuple(table[(B, k, 0.1)] for k in range(3)) == BIASED_START_1[B], B


def test_the_table_is_whole(table):
    assert len(table) == 2 * 3 * len(BIASES) and all(len(row) == 3 and all(isinstance(x, int) and x >= 0 for x in row) for row in table.values())
