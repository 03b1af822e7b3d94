"""The layout of a packed composite join key (mdb_dev_join_key_layout, include/mdb_dev.h): a pure host function - per column pair the
field is the intersection of the two sides' ranges, columns are taken in the order given while they fit 63 bits together, the first
taken column is the most significant.  No device is needed."""
import ctypes

I64_MIN, I64_MAX = -2**63, 2**63 - 1


def layout(left, right):
    from midoridb_amd.dev import join_key_layout
    return join_key_layout(left, right)


def fields(lay):
    return {k: lay[k] for k in ("ntaken", "total_bits", "empty", "taken", "lo", "span", "bits", "shift")}


def test_eight_by_five_thousand_values():
    lay = layout([(0, 7), (0, 4999)], [(0, 7), (0, 4999)])
    assert fields(lay) == {"ntaken": 2, "total_bits": 16, "empty": 0, "taken": [0, 1], "lo": [0, 0], "span": [7, 4999], "bits": [3, 13],
                           "shift": [13, 0]}
    # the same values somewhere else on the number line: lo moves, nothing else does
    lay = layout([(-3, 4), (10**12, 10**12 + 4999)], [(-3, 4), (10**12, 10**12 + 4999)])
    assert fields(lay) == {"ntaken": 2, "total_bits": 16, "empty": 0, "taken": [0, 1], "lo": [-3, 10**12], "span": [7, 4999], "bits": [3, 13],
                           "shift": [13, 0]}


def test_the_field_is_the_intersection_of_the_two_ranges():
    lay = layout([(0, 100), (5, 5)], [(50, 200), (5, 5)])
    assert lay["lo"] == [50, 5] and lay["span"] == [50, 0] and lay["bits"] == [6, 0] and lay["shift"] == [0, 0]
    assert lay["ntaken"] == 2 and lay["total_bits"] == 6 and not lay["empty"]
    # ... whichever side is the narrow one
    assert fields(layout([(50, 200), (5, 5)], [(0, 100), (5, 5)])) == fields(lay)


def test_disjoint_ranges_and_a_side_without_values_are_empty():
    assert layout([(0, 10), (0, 10)], [(0, 10), (11, 20)])["empty"] == 1
    assert layout([(0, 10), (20, 30)], [(0, 10), (0, 19)])["empty"] == 1
    assert layout([(0, 10), (0, -1)], [(0, 10), (0, 10)])["empty"] == 1           # min > max: no non-NULL value on the left
    assert layout([(0, 10), (0, 10)], [(I64_MAX, I64_MIN), (0, 10)])["empty"] == 1  # ... on the right, as mdb_dev_key_range reports it
    assert layout([(0, 10), (0, 10)], [(0, 10), (0, 10)])["empty"] == 0


def test_31_plus_32_bits_are_both_taken():
    lay = layout([(0, 2**31 - 1), (-2**31, 2**31 - 1)], [(0, 2**31 - 1), (-2**31, 2**31 - 1)])
    assert fields(lay) == {"ntaken": 2, "total_bits": 63, "empty": 0, "taken": [0, 1], "lo": [0, -2**31], "span": [2**31 - 1, 2**32 - 1],
                           "bits": [31, 32], "shift": [32, 0]}


def test_32_plus_32_bits_the_second_column_is_skipped():
    lay = layout([(0, 2**32 - 1), (0, 2**32 - 1)], [(0, 2**32 - 1), (0, 2**32 - 1)])
    assert lay["ntaken"] == 1 and lay["taken"] == [0] and lay["total_bits"] == 32 and not lay["empty"]      # < 2: not served


def test_a_middle_column_that_does_not_fit_is_skipped_and_the_next_one_taken():
    rng = [(0, 2**20 - 1), (0, 2**50), (0, 2**40 - 1)]
    lay = layout(rng, rng)
    assert fields(lay) == {"ntaken": 2, "total_bits": 60, "empty": 0, "taken": [0, 2], "lo": [0, 0], "span": [2**20 - 1, 2**40 - 1],
                           "bits": [20, 40], "shift": [40, 0]}


def test_the_whole_int64_range_is_never_taken_and_nothing_overflows():
    full = (I64_MIN, I64_MAX)
    lay = layout([full, full], [full, full])
    assert lay["ntaken"] == 0 and lay["total_bits"] == 0 and not lay["empty"]
    # next to columns that fit it is skipped; its neighbours at the ends of the number line are exact
    lay = layout([full, (I64_MIN, I64_MIN + 2**31 - 1), (I64_MAX - 2**32 + 1, I64_MAX)], [full, (I64_MIN, I64_MAX), (0, I64_MAX)])
    assert fields(lay) == {"ntaken": 2, "total_bits": 63, "empty": 0, "taken": [1, 2], "lo": [I64_MIN, I64_MAX - 2**32 + 1],
                           "span": [2**31 - 1, 2**32 - 1], "bits": [31, 32], "shift": [32, 0]}
    # one value short of the whole range: 2^64 - 2 still has 64 bits
    assert layout([(I64_MIN, I64_MAX - 1), (0, 1)], [(I64_MIN, I64_MAX), (0, 1)])["taken"] == [1]
    # [INT64_MIN, -1] against [0, INT64_MAX]: disjoint, no overflow in finding that out
    assert layout([(I64_MIN, -1), (0, 1)], [(0, I64_MAX), (0, 1)])["empty"] == 1


def test_at_most_four_columns_are_taken():
    rng = [(0, 3)] * 6
    lay = layout(rng, rng)
    assert lay["ntaken"] == 4 and lay["taken"] == [0, 1, 2, 3] and lay["shift"] == [6, 4, 2, 0] and lay["total_bits"] == 8


def test_composite_join_counter_exists_and_starts_at_zero():
    from midoridb_amd.query import DB
    with DB() as db:
        assert db.composite_joins() == 0
        assert isinstance(db.lib.mdb_database_composite_joins(ctypes.byref(db.db)), int)
