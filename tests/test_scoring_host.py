"""Host side of the shared scoring run (crossscore_amd/scoring.py, data.py): which files a batch reads, the decode window's plan, the host
decode and the collated item paths, on hand-made item dictionaries.  No GPU."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from crossscore_amd import data as csdata  # noqa: E402

E = csdata.EMPTY


def _item(q, refs):
    return {"query/img": q, "query/score_map": q.replace("q", "m"), "reference/cross/imgs": list(refs)}


# two batches of two items, three references each: one EMPTY slot (q1), and r2 shared across the batches (q0 and q3)
BATCHES = [[_item("q0", ("r0", "r1", "r2")), _item("q1", ("r3", E, "r4"))],
           [_item("q2", ("r5", "r6", "r7")), _item("q3", ("r2", "r8", "r9"))]]


def _rgb(paths):
    return [(p, False) for p in paths]


def test_batch_files_order_and_placeholders():
    assert csdata.batch_files(BATCHES[0]) == _rgb(["q0", "r0", "r1", "r2", "q1", "r3", "r4"])  # query first, slots in order, EMPTY skipped
    assert csdata.batch_files(BATCHES[1]) == _rgb(["q2", "r5", "r6", "r7", "q3", "r2", "r8", "r9"])
    assert csdata.batch_files(BATCHES[0], zero_reference=True) == _rgb(["q0", "q1"])
    assert csdata.batch_files(BATCHES[1], skip={"r2", "q2"}) == _rgb(["q2", "r5", "r6", "r7", "q3", "r8", "r9"])  # skip names references only


def test_plan_decodes_lists_each_batch():
    plan = csdata.plan_decodes(BATCHES, False, False)
    assert plan == [csdata.batch_files(b) for b in BATCHES]
    assert csdata.plan_decodes(BATCHES, True, False) == [_rgb(["q0", "q1"]), _rgb(["q2", "q3"])]
    assert csdata.plan_decodes(BATCHES, True, True) == [_rgb(["q0", "q1"]), _rgb(["q2", "q3"])]
    once = csdata.plan_decodes(BATCHES, False, True)
    assert once[0] == plan[0]  # the first batch that names r2 reads it
    assert once[1] == _rgb(["q2", "r5", "r6", "r7", "q3", "r8", "r9"])  # the second finds its tokens: r2 dropped, and only r2


def test_plan_decodes_extra_follows_its_item():
    def extra(it):  # a 16-bit map per item, none for q1; q2 adds an 8-bit file too
        if it["query/img"] == "q1":
            return []
        return [(it["query/score_map"], True)] + ([("g2", False)] if it["query/img"] == "q2" else [])

    plan = csdata.plan_decodes(BATCHES, False, True, extra)
    assert plan[0] == _rgb(["q0", "r0", "r1", "r2"]) + [("m0", True)] + _rgb(["q1", "r3", "r4"])
    assert plan[1] == _rgb(["q2", "r5", "r6", "r7"]) + [("m2", True), ("g2", False)] + _rgb(["q3", "r8", "r9"]) + [("m3", True)]
    assert csdata.plan_decodes(BATCHES, True, False, extra)[0] == [("q0", False), ("m0", True), ("q1", False)]


def test_decode_items_reads_what_the_plan_lists(monkeypatch):
    read = []
    monkeypatch.setattr(csdata, "read_image_u8", lambda p: read.append(p) or ("img", p))
    twice = [BATCHES[0][0], _item("q4", ("r2", "r0", E))]  # r0 and r2 named by both items
    for items in (BATCHES[0], BATCHES[1], twice):
        del read[:]
        decoded = csdata.decode_items(items)
        assert len(read) == len(set(read))  # each path once
        assert set(read) == set(decoded) == {p for p, _ in csdata.plan_decodes([items], False, False)[0]}
        assert all(decoded[p] == ("img", p) for p in read)
    del read[:]
    decoded = csdata.decode_items(BATCHES[1], skip={"r2", "r8"})
    assert read == ["q2", "r5", "r6", "r7", "q3", "r9"] and list(decoded) == read
    del read[:]
    assert list(csdata.decode_items(BATCHES[0], zero_reference=True)) == ["q0", "q1"] == read


def test_item_paths_collates_references_slot_major():
    paths = csdata.item_paths(BATCHES[0])
    assert paths["query/img"] == ["q0", "q1"] and paths["query/score_map"] == ["m0", "m1"]
    assert paths["reference/cross/imgs"] == [["r0", "r3"], ["r1", E], ["r2", "r4"]]  # N lists of B paths, as default_collate gives
    assert csdata.item_paths([_item("q0", ())])["reference/cross/imgs"] == []


def test_decode_items_reads_extras_with_their_reader(monkeypatch):
    read8, read16 = [], []
    monkeypatch.setattr(csdata, "read_image_u8", lambda p: read8.append(p) or ("img", p))
    monkeypatch.setattr(csdata, "read_metric_map_u16", lambda p: read16.append(p) or ("map", p))

    def extra(it):  # as in test_plan_decodes_extra_follows_its_item, and q3 names r2 -- one of its own references -- as an 8-bit extra
        if it["query/img"] == "q1":
            return []
        return [(it["query/score_map"], True)] + ([("g2", False)] if it["query/img"] == "q2" else []) + ([("r2", False)] if it["query/img"] == "q3" else [])

    decoded = csdata.decode_items(BATCHES[0], extra=extra)
    assert read16 == ["m0"] and read8 == ["q0", "r0", "r1", "r2", "q1", "r3", "r4"]  # 16-bit entries to the map reader, the rest to the image reader
    assert list(decoded) == ["q0", "r0", "r1", "r2", "m0", "q1", "r3", "r4"] and decoded["m0"] == ("map", "m0") and decoded["r2"] == ("img", "r2")
    del read8[:], read16[:]
    decoded = csdata.decode_items(BATCHES[1], extra=extra)
    assert read16 == ["m2", "m3"] and read8 == ["q2", "r5", "r6", "r7", "g2", "q3", "r2", "r8", "r9"]  # r2: reference and extra, read once
    assert len(decoded) == len(read8) + len(read16)
    del read8[:], read16[:]
    decoded = csdata.decode_items(BATCHES[1], skip={"r2", "r8"}, extra=extra)  # a skipped reference that is also an extra is still read
    assert read16 == ["m2", "m3"] and read8 == ["q2", "r5", "r6", "r7", "g2", "q3", "r9", "r2"]
    assert decoded["r2"] == ("img", "r2") and "r8" not in decoded
    del read8[:], read16[:]
    assert list(csdata.decode_items(BATCHES[0], zero_reference=True, extra=extra)) == ["q0", "m0", "q1"] and read16 == ["m0"] and read8 == ["q0", "q1"]
