"""The count-all CPU oracle of the topology report (topology_cases.count_all) on the hand case where its classes differ from
the other stages'."""
import topology_cases as tc


def test_classification_follows_the_rotation_order():
    p, tri = tc.classification_trap()
    r = tc.count_all(len(p), tri)
    tc.assert_trap_report(r)                # (1, 1, 7) degenerate, (7, 2, 2) out of range, (3, 3, 3) degenerate
    assert r["count"][2:] == [0, 0, 0, 0]   # the square's four vertices are used and sound
