"""Holds tests/launch_caps_np.py to the sources, without a device: every row's literal still stands in the body of its launcher, every
clamp a source search finds is a row, and no row is blank.  A failure names the GPU test whose operands were sized against the old cap."""
import os

import launch_caps_np as lc


def _text(name):
    with open(os.path.join(lc.CSRC, name)) as f:
        return f.read()


def test_every_cap_still_stands_in_the_body_of_its_launcher():
    seen = {}
    for r in lc.TABLE:
        seen.setdefault((r["file"], r["launcher"], r["cap"]), []).append(r)
    for (file, launcher, cap), rows in seen.items():
        body = lc.body_of(_text(file), launcher)
        assert body is not None, f"{file}: no function {launcher} any more; its rows name {[r['test'] or 'no test' for r in rows]}"
        sized = sorted({r["test"] for r in rows if r["test"]}) or ["no GPU test (unreachable in seconds)"]
        assert lc.count_literal(body, cap) >= len(rows), (
            f"{file}: {launcher} no longer clamps to {cap}.  Sized against that cap: {', '.join(sized)} - "
            f"grow its operands past the new cap and update tests/launch_caps_np.py")


def test_every_clamp_of_the_sources_is_a_row():
    hits = lc.find_clamps()
    assert len(hits) >= len(lc.TABLE) - 1  # (col_scale_launch's two clamps are two hits; the search is not blind)
    unmatched = []
    counted = {}
    for file, header, line, cap in hits:
        if any(f == file and lc.header_names(header, fn) for (f, fn) in lc.NOT_CLAMPS):
            continue
        rows = [r for r in lc.TABLE if r["file"] == file and r["cap"] == cap and lc.header_names(header, r["launcher"])]
        if not rows:
            unmatched.append(f"{file}:{line} clamps to {cap} in `{header.strip()}`")
            continue
        key = (file, rows[0]["launcher"], cap)
        counted[key] = counted.get(key, 0) + 1
    assert not unmatched, "clamps without a row in tests/launch_caps_np.py:\n" + "\n".join(unmatched)
    # as many rows as clamps in every launcher
    for (file, launcher, cap), n in counted.items():
        assert len([r for r in lc.TABLE if (r["file"], r["launcher"], r["cap"]) == (file, launcher, cap)]) == n, (file, launcher, cap, n)
    assert len(counted) == len({(r["file"], r["launcher"], r["cap"]) for r in lc.TABLE})


def test_the_table_has_no_blanks():
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    for r in lc.TABLE:
        assert all(r[k] not in (None, "") for k in ("file", "launcher", "capped", "cap", "threads", "per_trip", "entry")), r
        assert r["capped"] in ("grid x", "grid y", "threads") and r["cap"] in lc.CAPS
        assert (r["test"] is None) != (r["reason"] is None), f"{r['launcher']}: exactly one of a test and a reason"
        if r["test"]:
            module, name = r["test"].split("::")
            with open(os.path.join(tests_dir, module)) as f:
                assert f"def {name}(" in f.read(), f"{r['launcher']}: {r['test']} does not exist"
        else:
            assert len(r["reason"]) > 20
        # a workgroup of a capped grid handles one item, or one per thread (rrlu_global_blocks: 1024 per workgroup)
        assert r["per_trip"] in ((r["cap"], r["cap"] * r["threads"], r["cap"] * 1024) if r["capped"] == "grid x" else (r["cap"],)), r


def test_the_parser_reads_the_forms_it_has_to():
    text = "namespace {\nunsigned f(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 4096); } // c\n}\nvoid g(int a,\n       int b);\n" \
           "void T::h(int a,\n          int b)\n{\n    if (b > 1024) b = 1024;\n    int c = a < 8192 ? a : 8192;\n}\nint k() { return 1; }\n"
    assert lc.count_literal(lc.body_of(text, "f"), 4096) == 1 and lc.body_of(text, "g") is None
    body = lc.body_of(text, "T::h")
    assert lc.count_literal(body, 1024) == 2 and lc.count_literal(body, 8192) == 2 and "k()" not in body
    assert lc.body_of(text, "h") is not None and lc.body_of(text, "T") is None
    assert lc.count_literal("x = 10240; y = 1024.5; z = a1024;", 1024) == 0
