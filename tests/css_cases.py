"""Document pairs for the stylesheet and document-structure tests: (name, styled document, plain document).  The styled one uses
<style> rules, ``display`` / ``visibility``, <symbol>, <switch> or <a>; the plain one spells the same picture with presentation
attributes, inline styles and ``<g transform clip-path>`` only, so that both must load to the same scene.  Every document is
64 x 64 user units.  OPTIONS: the extra loader arguments (``css=``, ``languages=``) a styled document is loaded with.
NEEDS_DEVICE: the pairs whose scene dump asks the device (marker vertices, dashes).  GPU_DOZEN: one pair per construct (and the filter pair), rendered
on the device."""

_XMLNS = 'xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink"'


def _doc(body, attrs=""):
    return f'<svg {_XMLNS} width="64" height="64"{attrs}>{body}</svg>'


# a three-glyph SVG font, for the pairs that set text (a: a square, b: a triangle, c: a bar); 1000 units per em
FONT = ('<defs><font id="face" horiz-adv-x="600"><font-face font-family="Blocks" units-per-em="1000" ascent="800" descent="-200"/>'
        '<glyph unicode="a" glyph-name="a" d="M50,0 H550 V500 H50 z"/><glyph unicode="b" glyph-name="b" d="M50,0 L550,0 L300,700 z"/>'
        '<glyph unicode="c" glyph-name="c" horiz-adv-x="300" d="M50,0 H250 V700 H50 z"/><glyph unicode=" " horiz-adv-x="300"/></font></defs>')

_ARROW = '<marker id="arrow" markerWidth="4" markerHeight="4" refX="2" refY="2" orient="auto"><path d="M0,0 L4,2 L0,4 z" fill="#c00"/></marker>'

# a symbol with a viewBox and two children, one of them hanging out of the viewBox on the right
_SYMBOL_BODY = '<rect x="2" y="2" width="8" height="8" fill="#06c"/><circle cx="14" cy="8" r="5" fill="#c60"/>'
_FRAME_16 = '<clipPath id="frame"><path d="M0,0 L16,0 L16,16 L0,16 z" fill="white"/></clipPath>'

CASES = [
    ("selectors_class_id_type_universal",
     _doc('<style>.c { fill: #c00 } #i { fill: #0c0 } circle { fill: #00c } * { stroke: #222 }</style>'
          '<rect class="c" x="4" y="4" width="20" height="20"/><rect id="i" x="30" y="4" width="20" height="20"/>'
          '<circle cx="20" cy="44" r="12"/>'),
     _doc('<rect x="4" y="4" width="20" height="20" fill="#c00" stroke="#222"/>'
          '<rect id="i" x="30" y="4" width="20" height="20" fill="#0c0" stroke="#222"/>'
          '<circle cx="20" cy="44" r="12" fill="#00c" stroke="#222"/>')),
    ("attribute_operators",
     _doc('<style>[data-k] { fill: #100 } [data-k=v] { stroke: #010 } [data-w~="b"] { fill: #200 } [lang|=en] { fill: #300 }'
          ' [data-p^=ab] { fill: #400 } [data-p$=\'yz\'] { fill: #500 } [data-p*=mid] { fill: #600 } [href] { fill: #700 }'
          ' [data-w~="a b"] { fill: #fff } [data-p^=""] { fill: #fff }</style>'
          '<rect id="r" data-k="u" x="0" y="0" width="8" height="8"/><rect data-k="v" x="8" y="0" width="8" height="8"/>'
          '<rect data-w="a b c" x="16" y="0" width="8" height="8"/><rect lang="en-GB" x="24" y="0" width="8" height="8"/>'
          '<rect lang="english" x="32" y="0" width="8" height="8"/><rect data-p="abc" x="0" y="8" width="8" height="8"/>'
          '<rect data-p="xyz" x="8" y="8" width="8" height="8"/><rect data-p="a-mid-z" x="16" y="8" width="8" height="8"/>'
          '<use xlink:href="#r" x="24" y="8"/>'),
     _doc('<rect id="r" x="0" y="0" width="8" height="8" fill="#100"/><rect x="8" y="0" width="8" height="8" fill="#100" stroke="#010"/>'
          '<rect x="16" y="0" width="8" height="8" fill="#200"/><rect x="24" y="0" width="8" height="8" fill="#300"/>'
          '<rect x="32" y="0" width="8" height="8"/><rect x="0" y="8" width="8" height="8" fill="#400"/>'
          '<rect x="8" y="8" width="8" height="8" fill="#500"/><rect x="16" y="8" width="8" height="8" fill="#600"/>'
          '<use xlink:href="#r" x="24" y="8" fill="#700"/>')),
    ("combinators",
     _doc('<style>g rect { fill: #c00 } g > rect { stroke: #00c } rect + circle { fill: #0c0 } rect ~ path { fill: #cc0 }'
          ' svg > g > g circle { stroke: #222 }</style>'
          '<rect x="0" y="0" width="8" height="8"/><g><rect x="10" y="0" width="8" height="8"/>'
          '<g><rect x="20" y="0" width="8" height="8"/><circle cx="34" cy="4" r="4"/><circle cx="44" cy="4" r="4"/>'
          '<path d="M0,20 L10,20 L5,30 z"/></g><path d="M20,20 L30,20 L25,30 z"/></g>'),
     _doc('<rect x="0" y="0" width="8" height="8"/><g><rect x="10" y="0" width="8" height="8" fill="#c00" stroke="#00c"/>'
          '<g><rect x="20" y="0" width="8" height="8" fill="#c00" stroke="#00c"/><circle cx="34" cy="4" r="4" fill="#0c0" stroke="#222"/>'
          '<circle cx="44" cy="4" r="4" stroke="#222"/><path d="M0,20 L10,20 L5,30 z" fill="#cc0"/></g>'
          '<path d="M20,20 L30,20 L25,30 z" fill="#cc0"/></g>')),
    ("structural_pseudo_classes",
     _doc('<style>rect:nth-child(2n+1) { fill: #c00 } rect:not(.x) { stroke: #00c } circle:first-of-type { fill: #0c0 }'
          ' rect:hover { fill: #fff } rect::before { fill: #fff } :root { stroke-width: 2 }</style>'
          '<g><rect x="0" y="0" width="8" height="8"/><rect class="x" x="10" y="0" width="8" height="8"/>'
          '<rect x="20" y="0" width="8" height="8"/><circle cx="34" cy="4" r="4"/><rect class="x y" x="40" y="0" width="8" height="8"/>'
          '<circle cx="54" cy="4" r="4"/></g>'),
     _doc('<g stroke-width="2"><rect x="0" y="0" width="8" height="8" fill="#c00" stroke="#00c"/><rect x="10" y="0" width="8" height="8"/>'
          '<rect x="20" y="0" width="8" height="8" fill="#c00" stroke="#00c"/><circle cx="34" cy="4" r="4" fill="#0c0"/>'
          '<rect x="40" y="0" width="8" height="8" fill="#c00"/><circle cx="54" cy="4" r="4"/></g>')),
    ("specificity_then_source_order",
     _doc('<style>.a { fill: #c00 } .b { fill: #00c } rect.a { stroke: #0c0 } .a { stroke: #cc0 } #q { fill: #0cc } .a.b { fill: #c0c }</style>'
          '<rect class="b a" x="4" y="4" width="20" height="20"/><rect class="a" x="30" y="4" width="20" height="20"/>'
          '<rect id="q" class="a b" x="4" y="30" width="20" height="20"/>'),
     _doc('<rect x="4" y="4" width="20" height="20" fill="#c0c" stroke="#0c0"/><rect x="30" y="4" width="20" height="20" fill="#c00" stroke="#0c0"/>'
          '<rect id="q" x="4" y="30" width="20" height="20" fill="#0cc" stroke="#0c0"/>')),
    ("rule_beats_presentation_attribute",
     _doc('<style>.k { fill: #0a0 } rect { stroke-width: 3 }</style>'
          '<rect class="k" fill="#c00" stroke="#222" stroke-width="1" x="8" y="8" width="40" height="40"/>'),
     _doc('<rect fill="#0a0" stroke="#222" stroke-width="3" x="8" y="8" width="40" height="40"/>')),
    ("inline_style_beats_rule",
     _doc('<style>#only.k { fill: #0a0; stroke: #222 }</style>'
          '<rect id="only" class="k" style="fill: #00c" x="8" y="8" width="40" height="40"/>'),
     _doc('<rect id="only" fill="#00c" stroke="#222" x="8" y="8" width="40" height="40"/>')),
    ("important",
     _doc('<style>.k { fill: #0a0 !important; stroke: #c00 ! IMPORTANT } #one { fill: #123 }</style>'
          '<rect id="one" class="k" style="fill: #00c; stroke: #222 !important" x="8" y="8" width="40" height="40"/>'),
     _doc('<rect id="one" fill="#0a0" stroke="#222" x="8" y="8" width="40" height="40"/>')),
    ("media_screen_and_print",
     _doc('<style>@media screen { .m { fill: #0a0 } } @media print { .m { fill: #c00 } } @media only all { .m { stroke: #222 } }'
          ' @media (min-width: 100px) { .m { stroke: #c00 } }</style><rect class="m" x="8" y="8" width="40" height="40"/>'),
     _doc('<rect fill="#0a0" stroke="#222" x="8" y="8" width="40" height="40"/>')),
    ("style_after_the_elements",
     _doc('<rect class="late" x="8" y="8" width="40" height="40"/><g><style>.late { fill: #0a0 }</style></g>'),
     _doc('<rect fill="#0a0" x="8" y="8" width="40" height="40"/><g/>')),
    ("cdata",
     _doc('<style type="text/css"><![CDATA[ g > .c { fill: #0a0 } /* a > b in a comment */ ]]></style>'
          '<g><rect class="c" x="8" y="8" width="40" height="40"/></g>'),
     _doc('<g><rect fill="#0a0" x="8" y="8" width="40" height="40"/></g>')),
    ("two_style_elements",
     _doc('<style>.t { fill: #c00; stroke: #222 }</style><rect class="t" x="8" y="8" width="40" height="40"/><style>.t { fill: #0a0 }</style>'
          '<style type="text/x-scss">.t { fill: #fff }</style>'),
     _doc('<rect fill="#0a0" stroke="#222" x="8" y="8" width="40" height="40"/>')),
    ("selector_list_with_an_invalid_selector",
     _doc('<style>.t, rect:frobnicate { fill: #c00 } rect { stroke: #222 }</style><rect class="t" x="8" y="8" width="40" height="40"/>'),
     _doc('<rect stroke="#222" x="8" y="8" width="40" height="40"/>')),
    ("gradient_stops_by_class",
     _doc('<style>.st0 { stop-color: #c00 } .st1 { stop-color: #00c; stop-opacity: 0.5 } .st2 { fill: url(#lg) }</style>'
          '<defs><linearGradient id="lg"><stop class="st0" offset="0"/><stop class="st1" offset="1" stop-color="#fff"/></linearGradient></defs>'
          '<rect class="st2" x="8" y="8" width="48" height="48"/>'),
     _doc('<defs><linearGradient id="lg"><stop stop-color="#c00" offset="0"/><stop offset="1" stop-color="#00c" stop-opacity="0.5"/></linearGradient></defs>'
          '<rect fill="url(#lg)" x="8" y="8" width="48" height="48"/>')),
    ("flood_color_by_class",
     _doc('<style>.fl { flood-color: #0a0; flood-opacity: 0.5 } .f { filter: url(#f) }</style>'
          '<filter id="f" x="0" y="0" width="1" height="1"><feFlood class="fl" flood-color="#c00"/></filter>'
          '<rect class="f" x="8" y="8" width="40" height="40"/>'),
     _doc('<filter id="f" x="0" y="0" width="1" height="1"><feFlood flood-color="#0a0" flood-opacity="0.5"/></filter>'
          '<rect filter="url(#f)" x="8" y="8" width="40" height="40"/>')),
    ("tspan_font_size_and_fill_by_class",
     _doc(FONT + '<style>.big { font-size: 24px; fill: #c00 } text { font-family: Blocks }</style>'
          '<text x="2" y="40" font-size="12">ab<tspan class="big">c a</tspan>b</text>'),
     _doc(FONT + '<text x="2" y="40" font-size="12" font-family="Blocks">ab<tspan font-size="24px" fill="#c00">c a</tspan>b</text>')),
    ("marker_end_by_class",
     _doc(_ARROW + '<style>.arrowed { marker-end: url(#arrow); stroke: #222; fill: none }</style><path class="arrowed" d="M8,8 L40,8 L40,40"/>'),
     _doc(_ARROW + '<path marker-end="url(#arrow)" stroke="#222" fill="none" d="M8,8 L40,8 L40,40"/>')),
    ("stroke_dasharray_by_rule",
     _doc('<style>path { stroke-dasharray: 6 3; stroke-dashoffset: 2; stroke: #222; fill: none; stroke-width: 2 }</style><path d="M8,8 L56,8 L56,56"/>'),
     _doc('<path stroke-dasharray="6 3" stroke-dashoffset="2" stroke="#222" fill="none" stroke-width="2" d="M8,8 L56,8 L56,56"/>')),
    ("inherit",
     _doc('<style>.i { fill: inherit; opacity: inherit; stroke-width: INHERIT }</style>'
          '<g fill="#c00" opacity="0.5" stroke="#222" stroke-width="3"><rect class="i" fill="#00c" stroke-width="1" x="8" y="8" width="40" height="40"/></g>'),
     _doc('<g fill="#c00" opacity="0.5" stroke="#222" stroke-width="3"><rect opacity="0.5" x="8" y="8" width="40" height="40"/></g>')),
    ("css_argument_wins_at_equal_specificity",
     _doc('<style>.t { fill: #c00; stroke: #222 }</style><rect class="t" x="8" y="8" width="40" height="40"/>'),
     _doc('<rect fill="#0a0" stroke="#222" x="8" y="8" width="40" height="40"/>')),
    ("display_none_on_a_group",
     _doc('<style>.off { display: none }</style><rect x="4" y="4" width="20" height="20" fill="#06c"/>'
          '<g class="off"><rect x="30" y="30" width="20" height="20" fill="#c00"/></g><circle display="NONE" cx="10" cy="50" r="8"/>'),
     _doc('<rect x="4" y="4" width="20" height="20" fill="#06c"/>')),
    ("display_none_on_a_use_target",
     _doc('<style>#t { display: none }</style><rect x="4" y="4" width="20" height="20" fill="#06c"/>'
          '<g id="t"><rect x="30" y="30" width="20" height="20" fill="#c00"/></g><use xlink:href="#t" x="-20" y="0"/>'),
     _doc('<rect x="4" y="4" width="20" height="20" fill="#06c"/>')),
    ("display_none_on_a_tspan",
     _doc(FONT + '<style>.off { display: none }</style><text x="2" y="40" font-size="12" font-family="Blocks">ab<tspan class="off" dx="20">ca</tspan>b</text>'),
     _doc(FONT + '<text x="2" y="40" font-size="12" font-family="Blocks">ab<tspan></tspan>b</text>')),
    ("display_none_on_a_child_of_a_clip_path",
     _doc('<style>.off { display: none }</style><clipPath id="c" display="none"><rect class="off" x="0" y="0" width="64" height="64"/><circle cx="32" cy="32" r="16"/></clipPath>'
          '<rect clip-path="url(#c)" x="8" y="8" width="48" height="48" fill="#06c"/>'),
     _doc('<clipPath id="c"><circle cx="32" cy="32" r="16"/></clipPath><rect clip-path="url(#c)" x="8" y="8" width="48" height="48" fill="#06c"/>')),
    ("visibility_hidden_with_a_visible_grandchild",
     _doc('<style>.hid { visibility: hidden } .vis { visibility: visible }</style>'
          '<g class="hid"><rect x="4" y="4" width="20" height="20" fill="#c00"/><g><rect class="vis" x="30" y="30" width="20" height="20" fill="#06c"/>'
          '<circle cx="12" cy="50" r="8" visibility="collapse"/></g></g>'),
     _doc('<g><g><rect x="30" y="30" width="20" height="20" fill="#06c"/></g></g>')),
    ("symbol_at_1x",
     _doc(f'<symbol id="sym" viewBox="0 0 16 16">{_SYMBOL_BODY}</symbol><use xlink:href="#sym" x="8" y="8" width="16" height="16"/>'),
     _doc(f'{_FRAME_16}<g transform="translate(8, 8)" clip-path="url(#frame)">{_SYMBOL_BODY}</g>')),
    ("symbol_at_2x",
     _doc(f'<symbol id="sym" viewBox="0 0 16 16">{_SYMBOL_BODY}</symbol><use xlink:href="#sym" x="8" y="8" width="32" height="32"/>'),
     _doc(f'{_FRAME_16}<g transform="translate(8, 8) scale(2)" clip-path="url(#frame)">{_SYMBOL_BODY}</g>')),
    # viewBox 8 x 16 sliced into 16 x 8: scale max(16 / 8, 8 / 16) = 2, xMin: no shift, YMax: shifted by 8 - 32 = -24; the viewport is
    # x in [0, 8], y in [24 / 2, 32 / 2] = [12, 16] of the content
    ("symbol_sliced_xMinYMax",
     _doc('<symbol id="sym" viewBox="0 0 8 16" preserveAspectRatio="xMinYMax slice"><rect x="1" y="1" width="6" height="14" fill="#06c"/>'
          '<circle cx="4" cy="14" r="3" fill="#c60"/></symbol><use xlink:href="#sym" x="16" y="24" width="16" height="8"/>'),
     _doc('<clipPath id="frame"><path d="M0,12 L8,12 L8,16 L0,16 z" fill="white"/></clipPath>'
          '<g transform="translate(16, 24) translate(0, -24) scale(2)" clip-path="url(#frame)"><rect x="1" y="1" width="6" height="14" fill="#06c"/>'
          '<circle cx="4" cy="14" r="3" fill="#c60"/></g>')),
    ("symbol_overflow_visible",
     _doc('<symbol id="sym" viewBox="0 0 16 16" overflow="visible"><circle cx="14" cy="8" r="5" fill="#c60"/></symbol>'
          '<use xlink:href="#sym" x="8" y="8" width="32" height="32"/>'),
     _doc('<g transform="translate(8, 8) scale(2)"><circle cx="14" cy="8" r="5" fill="#c60"/></g>')),
    ("symbol_without_any_size",
     _doc(f'<symbol id="sym" viewBox="0 0 16 16">{_SYMBOL_BODY}</symbol><use xlink:href="#sym" x="8" y="8"/>'),
     _doc(f'{_FRAME_16}<g transform="translate(8, 8)" clip-path="url(#frame)">{_SYMBOL_BODY}</g>')),
    ("use_of_an_svg_with_a_size",
     _doc('<svg id="n" x="2" y="2" width="16" height="16" viewBox="0 0 8 8"><rect x="1" y="1" width="7" height="7" fill="#06c"/></svg>'
          '<use xlink:href="#n" x="24" y="8" width="32" height="32"/>'),
     _doc('<svg id="n" x="2" y="2" width="16" height="16" viewBox="0 0 8 8"><rect x="1" y="1" width="7" height="7" fill="#06c"/></svg>'
          '<g transform=" translate(24, 8)"><svg x="2" y="2" width="32" height="32" viewBox="0 0 8 8"><rect x="1" y="1" width="7" height="7" fill="#06c"/></svg></g>')),
    ("switch_drawio_label",
     _doc(FONT + '<g><rect x="4" y="4" width="56" height="40" fill="#eee" stroke="#222"/><switch>'
          '<foreignObject requiredExtensions="http://www.w3.org/1999/xhtml" width="56" height="40"><div xmlns="http://www.w3.org/1999/xhtml">abc</div></foreignObject>'
          '<text x="8" y="30" font-family="Blocks" font-size="12">abc</text></switch></g>'),
     _doc(FONT + '<g><rect x="4" y="4" width="56" height="40" fill="#eee" stroke="#222"/>'
          '<text x="8" y="30" font-family="Blocks" font-size="12">abc</text></g>')),
    ("switch_system_language",
     _doc('<switch transform="translate(4, 4)" opacity="0.5"><rect systemLanguage="fr, it" width="40" height="40" fill="#c00"/>'
          '<rect systemLanguage="" width="40" height="40" fill="#c0c"/>'
          '<rect systemLanguage="en-US, DE" width="40" height="40" fill="#0a0"/><rect width="40" height="40" fill="#00c"/></switch>'),
     _doc('<g transform="translate(4, 4)" opacity="0.5"><rect width="40" height="40" fill="#0a0"/></g>')),
    ("a_around_a_shape",
     _doc('<a xlink:href="https://example.org/" transform="translate(4, 4)" fill="#06c"><rect width="40" height="40"/><circle cx="50" cy="50" r="6"/></a>'),
     _doc('<g transform="translate(4, 4)" fill="#06c"><rect width="40" height="40"/><circle cx="50" cy="50" r="6"/></g>')),
    ("a_inside_text",
     _doc(FONT + '<text x="2" y="40" font-size="12" font-family="Blocks">ab<a xlink:href="#x" fill="#06c">c<tspan dy="-4">a</tspan></a>b</text>'),
     _doc(FONT + '<text x="2" y="40" font-size="12" font-family="Blocks">ab<tspan fill="#06c">c<tspan dy="-4">a</tspan></tspan>b</text>')),
]

OPTIONS = {
    "css_argument_wins_at_equal_specificity": dict(css=".t { fill: #0a0 }"),
    "switch_system_language": dict(languages=("de-CH",)),
}
NEEDS_DEVICE = ("marker_end_by_class", "stroke_dasharray_by_rule")
GPU_DOZEN = (
    "gradient_stops_by_class", "important", "display_none_on_a_group", "visibility_hidden_with_a_visible_grandchild", "symbol_at_1x",
    "symbol_at_2x", "symbol_sliced_xMinYMax", "symbol_overflow_visible", "symbol_without_any_size", "switch_drawio_label",
    "a_around_a_shape", "css_argument_wins_at_equal_specificity", "flood_color_by_class",
)
BY_NAME = {name: (styled, plain) for name, styled, plain in CASES}
