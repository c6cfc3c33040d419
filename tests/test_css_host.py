"""The stylesheet module on its own (svgrasterize.py_amd/css.py): what ``parse_css`` understands of a sheet that uses every token
form, selector specificities against hand-computed triples, malformed input (nothing raises, everything warns as documented), that
nothing is ever opened or fetched for style, and a 2000-rule sheet on a 2000-element document."""
import builtins
import socket
import warnings

import pytest


def parse(text):
    from svgrasterize_amd import parse_css

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sheet = parse_css(text)
    return sheet, [str(w.message) for w in caught]


SHEET = r"""@charset "utf-8";
@namespace svg url(http://www.w3.org/2000/svg);
<!-- /* a comment with { braces } and a ; */ -->
.a, #b > rect { fill: red; stroke : "x;}y" ; }
.c\.d, .st\30 { FILL: Blue !important }
svg|rect[data-x="}"] { fill: url("a;b") /* ; stroke: none */; stroke-width: 2 ! Important; }
.e { color: red; : bad; fill green; stroke: #111 }
@media screen, print and (color) { g   rect:nth-child( 2n + 1 ) { fill: #abc } }
@media print { .never { fill: red } }
.f { fill: red
"""


def test_rules_of_a_sheet_with_every_token_form():
    sheet, warned = parse(SHEET)
    ab = (("fill", "red", False), ("stroke", '"x;}y"', False))
    cd = (("fill", "Blue", True),)
    assert [tuple(r) for r in sheet.rules] == [
        (".a", (0, 1, 0), 0, ab),
        ("#b > rect", (1, 0, 1), 1, ab),
        (".c\\.d", (0, 1, 0), 2, cd),
        (".st\\30", (0, 1, 0), 3, cd),
        ('svg|rect[data-x="}"]', (0, 1, 1), 4, (("fill", 'url("a;b")', False), ("stroke-width", "2", True))),
        (".e", (0, 1, 0), 5, (("color", "red", False), ("stroke", "#111", False))),
        ("g rect:nth-child( 2n + 1 )", (0, 1, 2), 6, (("fill", "#abc", False),)),
        (".f", (0, 1, 0), 7, (("fill", "red", False),)),
    ]
    assert sum("malformed declaration" in w for w in warned) == 2
    assert sum("unclosed block" in w for w in warned) == 1
    assert sum("@media" in w for w in warned) == 1
    assert len(warned) == 4 and len(sheet) == 8


def test_escapes_and_strings_reach_the_matcher():
    """``.st\\30`` is the class ``st0``, ``.c\\.d`` the class ``c.d``, and a brace inside a quoted attribute value is a value."""
    import svgrasterize_amd as S

    doc = ('<svg xmlns="http://www.w3.org/2000/svg" width="8" height="8"><style>' + SHEET + '</style>'
           '<rect id="one" class="st0" width="1" height="1"/><rect id="two" class="c.d" width="1" height="1"/>'
           '<rect id="three" data-x="}" width="1" height="1"/></svg>')
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _scene, ids, _size = S.svg_scene_from_str(doc)
    blue = [0.0, 0.0, 1.0, 1.0]
    assert ids["one"][1][1].tolist() == blue and ids["two"][1][1].tolist() == blue   # (a FILL node: (path, paint, rule))
    assert all(ids[k][0] == S.RENDER_FILL for k in ("one", "two"))
    assert "three" not in ids   # the rule was read: fill: url("a;b") is no paint, so nothing is drawn (unmatched, it would be black)


# selector -> (ids, classes + attributes + pseudo-classes, types), worked out by hand from Selectors Level 3 section 9
SPECIFICITY = [
    ("*", (0, 0, 0)),
    ("rect", (0, 0, 1)),
    (".a", (0, 1, 0)),
    ("#i", (1, 0, 0)),
    ("rect.a", (0, 1, 1)),
    ("rect.a.b", (0, 2, 1)),
    ("#i.a", (1, 1, 0)),
    ("g rect", (0, 0, 2)),
    ("g > rect + circle ~ path", (0, 0, 4)),
    ("[href]", (0, 1, 0)),
    ("rect[data-k=v]", (0, 1, 1)),
    ('a[href^="http"][target]', (0, 2, 1)),
    (":root", (0, 1, 0)),
    ("rect:first-child", (0, 1, 1)),
    ("rect:nth-child(2n+1)", (0, 1, 1)),
    ("rect:nth-last-child(odd)", (0, 1, 1)),
    (":not(.x)", (0, 1, 0)),
    ("rect:not(#i)", (1, 0, 1)),
    (":not(rect)", (0, 0, 1)),
    ("*:not(*)", (0, 0, 0)),
    ("a:hover", (0, 1, 1)),
    ("rect::before", (0, 0, 2)),
    ("p:after", (0, 0, 2)),
    ("svg|rect", (0, 0, 1)),
    ("*|*", (0, 0, 0)),
    ("#a #b .c .d e f", (2, 2, 2)),
    ("g:first-of-type > rect.a:not(.b):last-child", (0, 4, 2)),
    (".st\\30", (0, 1, 0)),
]


@pytest.mark.parametrize("selector,want", SPECIFICITY, ids=[s for s, _ in SPECIFICITY])
def test_specificity(selector, want):
    sheet, warned = parse(selector + " { fill: red }")
    assert not warned and len(sheet.rules) == 1
    assert sheet.rules[0].specificity == want and sheet.rules[0].selector == selector


@pytest.mark.parametrize("selector", ["rect:frobnicate", "a:is(b)", "a:where(b)", "a:has(b)", "rect >", "> rect", "a,,b", "a:not(b c)",
                                      "a:not(:not(b))", "rect[]", "[a=]", "[a!=b]", "#1a", ".2b", "a::before.c", "a:nth-child(n n)", ""])
def test_an_invalid_selector_drops_its_whole_rule(selector):
    sheet, warned = parse(f".ok, {selector} {{ fill: red }} .after {{ fill: blue }}")
    assert [r.selector for r in sheet.rules] == [".after"]
    assert len(warned) == 1 and "rule dropped" in warned[0] and ".ok" in warned[0]


def test_malformed_input_raises_nothing_and_warns():
    sheet, warned = parse(".a { fill: red; .b { fill: blue }")   # an unclosed brace
    assert [r.selector for r in sheet.rules] == [".a"] and sheet.rules[0].declarations == (("fill", "red", False),)
    assert any("unclosed block" in w for w in warned) and any("malformed declaration" in w for w in warned)
    sheet, warned = parse("} .g { fill: red } }")                # stray closing braces
    assert [r.selector for r in sheet.rules] == [".g"] and sum("stray }" in w for w in warned) >= 1
    sheet, warned = parse('@import url(http://example.org/a.css); @import "b.css" screen; .h { fill: red }')
    assert [r.selector for r in sheet.rules] == [".h"] and warned == ["@import is not followed: nothing is fetched"]
    sheet, warned = parse("@font-face { font-family: x; src: url(y.woff) } @keyframes k { from { a: b } to { a: c } } @-webkit-keyframes k { }"
                          " @supports (display: grid) { .s { fill: red } } @page :first { margin: 0 } @foo bar { .z { fill: red } } @foo { }"
                          " .i { fill: red }")
    assert [r.selector for r in sheet.rules] == [".i"]
    assert sorted(warned) == sorted([f"stylesheet: @{kind} is not supported and skipped" for kind in ("font-face", "keyframes", "supports", "page")]
                                    + ["stylesheet: unknown at-rule @foo skipped"])
    for text in ("", "   ", "/* open comment", "{", "}{", "a{", "a{b", "a{b:", "a{b:c", '"', ".a{fill:'x", "@", "@media", "@media {", "\\", ".a\\", "a{b:c}}}}",
                 "[[[[", "((((", ".a { fill: red !important !important }", "\x00", ".a{" * 50):
        sheet, _warned = parse(text)
        assert isinstance(sheet.rules, list)   # (reached: nothing was raised)


def test_media_queries():
    for prelude, applies in (("", True), ("all", True), ("screen", True), ("only screen", True), ("print, screen", True), ("SCREEN", True),
                             ("print", False), ("not screen", False), ("screen and (min-width: 100px)", False), ("(color)", False),
                             ("not all, print", False)):
        sheet, warned = parse(f"@media {prelude} {{ .m {{ fill: red }} }}")
        assert (len(sheet.rules) == 1) == applies, prelude
        assert len(warned) == (0 if applies else 1), prelude


def test_sheets_add_up_in_source_order():
    from svgrasterize_amd import Stylesheet, parse_css

    both = parse_css(".a { fill: red } .b { fill: blue }") + parse_css(".a { fill: green }")
    assert isinstance(both, Stylesheet) and [(r.selector, r.index) for r in both.rules] == [(".a", 0), (".b", 1), (".a", 2)]


def test_nothing_is_opened_or_fetched_for_style(monkeypatch):
    """``@import``, ``<?xml-stylesheet?>`` and <link> name files and URLs; the loader reads none of them."""
    import svgrasterize_amd as S

    doc = ('<?xml version="1.0"?><?xml-stylesheet type="text/css" href="theme.css"?>'
           '<svg xmlns="http://www.w3.org/2000/svg" width="8" height="8"><link xmlns="http://www.w3.org/1999/xhtml" rel="stylesheet" href="http://example.org/a.css"/>'
           '<style>@import url(http://example.org/b.css); @import "local.css"; .a { fill: red }</style><rect id="r" class="a" width="4" height="4"/></svg>')

    def refuse(*_args, **_kwargs):
        raise AssertionError("the loader tried to open a file or a socket")

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        monkeypatch.setattr(builtins, "open", refuse)
        monkeypatch.setattr(socket, "socket", refuse)
        _scene, ids, _size = S.svg_scene_from_str(doc, css="@import url(http://example.org/c.css);")
        monkeypatch.undo()
    assert ids["r"][1][1].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert [str(w.message) for w in caught].count("@import is not followed: nothing is fetched") == 1   # (once per document)


def test_2000_rules_on_2000_elements_load():
    """The unfamiliar-document guard: without the matcher's index every element is tested against every rule (4 M selector
    matches); this is a completion check, not a timing assertion."""
    import svgrasterize_amd as S

    n = 2000
    rules = "".join(f"g > .c{i} {{ fill: #{i:06x} }}" for i in range(n))
    shapes = "".join(f'<rect class="c{i}" x="{i % 64}" y="{i // 64}" width="1" height="1"/>' for i in range(n))
    doc = f'<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64"><style>{rules}</style><g>{shapes}</g></svg>'
    scene, _ids, _size = S.svg_scene_from_str(doc)
    fills = scene[1][0][1]   # (TRANSFORM of the GROUP of the fills)
    assert len(fills) == n
    want = S.svg.parse_color(f"#{n - 1:06x}")
    assert fills[-1][1][1].tolist() == want.tolist() and fills[0][1][1].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_exports():
    import svgrasterize_amd as S

    assert all(name in S.__all__ for name in ("parse_css", "Stylesheet", "Symbol"))
