"""Stylesheets for the SVG front-end (beyond the reference): the part of CSS that SVG documents use -- ``parse_css`` (CSS Syntax
Level 3's error recovery, written by hand: comments, strings, escapes, qualified rules with selector lists, declarations with
``!important``, ``@media``), Selectors Level 3 without the namespaces and the dynamic states, and ``Matcher``, which finds the
declarations that apply to an element of an ``xml.etree`` document.  Host code that runs once per document load; no dependency.

A stylesheet never raises: a malformed declaration is skipped up to the next ``;``, a malformed rule up to its matching ``}``, an
invalid selector drops the rule it stands in (its whole selector list, as CSS says), and each says so in a warning.  What a sheet
was understood to say is ``Stylesheet.rules``.  Nothing is ever fetched: ``@import`` warns and does nothing.
"""
from __future__ import annotations

import re
import warnings
from typing import NamedTuple

# pseudo-classes that are valid and never match: nothing is hovered, focused or visited in a picture
_NEVER = {
    "hover", "focus", "active", "visited", "link", "any-link", "target", "checked", "enabled", "disabled", "indeterminate", "default",
    "focus-within", "focus-visible", "valid", "invalid", "required", "optional", "read-only", "read-write", "placeholder-shown",
    "in-range", "out-of-range",
}
_LEGACY_PSEUDO_ELEMENTS = {"before", "after", "first-line", "first-letter"}   # (may be written with one colon)
_SKIPPED_AT_RULES = {"font-face", "keyframes", "supports", "page"}
_IMPORTANT = re.compile(r"!\s*important\s*$", re.IGNORECASE)
_NTH = re.compile(r"([+-]?\d*)n(?:\s*([+-])\s*(\d+))?$")
_HEX_ESCAPE = re.compile(r"[0-9A-Fa-f]{1,6}")
_WHITE = " \t\n\r\f"


class Rule(NamedTuple):
    """One selector of a qualified rule with the rule's declarations.  `selector`: its text; `specificity` = (ids, classes +
    attributes + pseudo-classes, types); `index`: the place in the source order of the sheet; `declarations`: a tuple of
    ``(property, value, important)``, the property in lower case, the value as written."""

    selector: str
    specificity: tuple
    index: int
    declarations: tuple


class _Compound:
    """A compound selector: what one element has to be."""

    __slots__ = ("tag", "ids", "classes", "attrs", "pseudos", "nots", "never", "elements")

    def __init__(self):
        self.tag = None      # local name, None: any
        self.ids = []
        self.classes = []
        self.attrs = []      # (local name, operator or None, value)
        self.pseudos = []    # (name, argument): the structural pseudo-classes
        self.nots = []       # compounds of :not()
        self.never = 0       # dynamic pseudo-classes (count as classes) ...
        self.elements = 0    # ... and pseudo-elements (count as types): valid, never matching

    def specificity(self):
        a, b, c = len(self.ids), len(self.classes) + len(self.attrs) + len(self.pseudos) + self.never, (self.tag is not None) + self.elements
        for inner in self.nots:
            ia, ib, ic = inner.specificity()
            a, b, c = a + ia, b + ib, c + ic
        return a, b, c


class Stylesheet:
    """Parsed style rules in source order.  `rules`: ``Rule`` tuples (one per selector of a selector list).  Sheets add up with
    ``+``: the right one's rules come later in the source order, so at equal specificity they win."""

    def __init__(self, rules=(), selectors=()):
        self.rules = [r._replace(index=i) for i, r in enumerate(rules)]
        self._selectors = list(selectors)   # per rule: [(combinator to the right neighbour or None, _Compound)], rightmost first

    def __add__(self, other):
        if not isinstance(other, Stylesheet):
            return NotImplemented
        return Stylesheet(self.rules + other.rules, self._selectors + other._selectors)

    def __len__(self):
        return len(self.rules)

    def __repr__(self):
        return f"Stylesheet({len(self.rules)} rules)"


# ---------------------------------------------------------------------------------------------------------------------
# scanning
# ---------------------------------------------------------------------------------------------------------------------
def _strip_comments(text: str) -> str:
    """`text` with every comment replaced by a blank; ``/*`` inside a string is not a comment, an open comment ends the sheet."""
    if "/*" not in text:
        return text
    out, pos, n = [], 0, len(text)
    while pos < n:
        ch = text[pos]
        if ch in "\"'":
            end = _string_end(text, pos)
            out.append(text[pos:end])
            pos = end
        elif ch == "\\" and pos + 1 < n:
            out.append(text[pos:pos + 2])
            pos += 2
        elif ch == "/" and text.startswith("/*", pos):
            end = text.find("*/", pos + 2)
            out.append(" ")
            pos = n if end < 0 else end + 2
        else:
            out.append(ch)
            pos += 1
    return "".join(out)


def _string_end(text: str, pos: int) -> int:
    """The index after the string that starts at `pos` (a quote); an unescaped newline or the end of the text ends it too."""
    quote, pos, n = text[pos], pos + 1, len(text)
    while pos < n:
        ch = text[pos]
        if ch == "\\":
            pos += 2
            continue
        if ch == quote:
            return pos + 1
        if ch == "\n":
            return pos
        pos += 1
    return n


_CLOSERS = {"(": ")", "[": "]", "{": "}"}


def _scan(text: str, pos: int, stops: str) -> int:
    """The index of the first character of `stops` at or after `pos` that is outside strings, escapes and nested brackets;
    ``len(text)`` when there is none."""
    n, stack = len(text), []
    while pos < n:
        ch = text[pos]
        if ch == "\\":
            pos += 2
            continue
        if ch in "\"'":
            pos = _string_end(text, pos)
            continue
        if not stack and ch in stops:
            return pos
        if ch in _CLOSERS:
            stack.append(_CLOSERS[ch])
        elif stack and ch == stack[-1]:
            stack.pop()
        pos += 1
    return n


def _skip_white(text: str, pos: int) -> int:
    n = len(text)
    while pos < n and text[pos] in _WHITE:
        pos += 1
    return pos


def _escape(text: str, pos: int):
    """The character a backslash escape at `pos` (the backslash) stands for, and the index after it."""
    m = _HEX_ESCAPE.match(text, pos + 1)
    if m is not None:
        end = m.end()
        if end < len(text) and text[end] in _WHITE:
            end += 1
        code = int(m.group(), 16)
        return (chr(code) if 0 < code <= 0x10FFFF and not 0xD800 <= code <= 0xDFFF else "�"), end
    if pos + 1 >= len(text) or text[pos + 1] == "\n":
        return None, pos + 1
    return text[pos + 1], pos + 2


def _ident(text: str, pos: int):
    """An identifier at `pos`, backslash escapes resolved: ``(name, index after it)``, or ``(None, pos)``."""
    out, start, n = [], pos, len(text)
    while pos < n:
        ch = text[pos]
        if ch == "\\":
            got, end = _escape(text, pos)
            if got is None:
                break
            out.append(got)
            pos = end
        elif ch.isalnum() or ch in "-_" or ord(ch) >= 0x80:
            if not out and ch.isdigit():
                break
            out.append(ch)
            pos += 1
        else:
            break
    name = "".join(out)
    if not name or name == "-" or (name[0] == "-" and name[1].isdigit() and text[start] != "\\"):
        return None, start
    return name, pos


def _string_value(text: str) -> str:
    """What a quoted string (quotes included) says."""
    out, pos, end = [], 1, len(text) - 1 if len(text) > 1 and text[-1] == text[0] else len(text)
    while pos < end:
        ch = text[pos]
        if ch == "\\":
            if pos + 1 < end and text[pos + 1] == "\n":
                pos += 2
                continue
            got, pos = _escape(text, pos)
            if got is not None:
                out.append(got)
        else:
            out.append(ch)
            pos += 1
    return "".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# selectors
# ---------------------------------------------------------------------------------------------------------------------
class _Invalid(Exception):
    pass


def _parse_nth(text: str):
    """``an+b`` / ``odd`` / ``even`` -> (a, b)."""
    text = text.strip().lower()
    if text == "odd":
        return 2, 1
    if text == "even":
        return 2, 0
    m = _NTH.match(text)
    if m is not None:
        a = m.group(1)
        a = int(a + "1") if a in ("", "+", "-") else int(a)
        return a, 0 if m.group(3) is None else int(m.group(2) + m.group(3))
    try:
        if re.match(r"[+-]?\d+$", text) is None:
            raise ValueError(text)
        return 0, int(text)
    except ValueError:
        raise _Invalid(f"invalid an+b: {text}") from None


def _parse_compound(text: str, pos: int, inside_not=False):
    """A compound selector at `pos` -> (_Compound, index after it)."""
    comp, n, start = _Compound(), len(text), pos
    # the type selector, with an optional namespace prefix that is accepted and ignored
    if pos < n and (text[pos] == "*" or text[pos] == "|" or _ident(text, pos)[0] is not None):
        if text[pos] == "*":
            name, pos = "*", pos + 1
        elif text[pos] == "|":
            name = ""
        else:
            name, pos = _ident(text, pos)
        if pos < n and text[pos] == "|" and not text.startswith("|=", pos):
            pos += 1
            if pos < n and text[pos] == "*":
                name, pos = "*", pos + 1
            else:
                name, pos = _ident(text, pos)
                if name is None:
                    raise _Invalid("a name is expected after the namespace prefix")
        if name != "*":
            comp.tag = name
    seen_element = False
    while pos < n:
        ch = text[pos]
        if seen_element and ch in "#.[:":
            raise _Invalid("nothing may follow a pseudo-element")
        if ch == "#":
            name, end = _ident(text, pos + 1)
            if name is None:   # (a hash that is no identifier, "#1a", is no id selector)
                raise _Invalid("invalid id selector")
            comp.ids.append(name)
            pos = end
        elif ch == ".":
            name, end = _ident(text, pos + 1)
            if name is None:
                raise _Invalid("invalid class selector")
            comp.classes.append(name)
            pos = end
        elif ch == "[":
            end = _scan(text, pos + 1, "]")
            if end >= n:
                raise _Invalid("unclosed attribute selector")
            comp.attrs.append(_parse_attribute(text[pos + 1:end]))
            pos = end + 1
        elif ch == ":":
            double = text.startswith("::", pos)
            name, end = _ident(text, pos + (2 if double else 1))
            if name is None:
                raise _Invalid("invalid pseudo-class")
            name = name.lower()
            argument = None
            if end < n and text[end] == "(":
                close = _scan(text, end + 1, ")")
                if close >= n:
                    raise _Invalid("unclosed parenthesis")
                argument, end = text[end + 1:close], close + 1
            pos = end
            if double or (name in _LEGACY_PSEUDO_ELEMENTS and argument is None):
                if inside_not or (double and argument is not None):
                    raise _Invalid(f"invalid pseudo-element: {name}")
                comp.elements += 1
                seen_element = True
            elif name in _NEVER and argument is None:
                comp.never += 1
            elif name in ("root", "first-child", "last-child", "only-child", "first-of-type", "last-of-type") and argument is None:
                comp.pseudos.append((name, None))
            elif name in ("nth-child", "nth-last-child") and argument is not None:
                comp.pseudos.append((name, _parse_nth(argument)))
            elif name == "not" and argument is not None and not inside_not:
                inner, stop = _parse_compound(argument, _skip_white(argument, 0), inside_not=True)
                if _skip_white(argument, stop) != len(argument):
                    raise _Invalid(":not() takes one compound selector")
                comp.nots.append(inner)
            else:
                raise _Invalid(f"unsupported pseudo-class: {name}")
        else:
            break
    if pos == start:
        raise _Invalid("a selector is expected")
    return comp, pos


def _parse_attribute(text: str):
    """The inside of ``[...]`` -> (local name, operator or None, value)."""
    pos = _skip_white(text, 0)
    if text.startswith("*|", pos):
        pos += 2
    elif text.startswith("|", pos) and not text.startswith("|=", pos):
        pos += 1
    name, pos = _ident(text, pos)
    if name is None:
        raise _Invalid("an attribute name is expected")
    if text.startswith("|", pos) and not text.startswith("|=", pos):   # (a namespace prefix: accepted and ignored)
        name, pos = _ident(text, pos + 1)
        if name is None:
            raise _Invalid("an attribute name is expected")
    pos = _skip_white(text, pos)
    if pos == len(text):
        return name, None, None
    for op in ("=", "~=", "|=", "^=", "$=", "*="):
        if text.startswith(op, pos):
            pos = _skip_white(text, pos + len(op))
            break
    else:
        raise _Invalid("invalid attribute operator")
    if pos < len(text) and text[pos] in "\"'":
        end = _string_end(text, pos)
        if text[end - 1] != text[pos] or end - pos < 2:
            raise _Invalid("unclosed string")
        value = _string_value(text[pos:end])
    else:
        value, end = _ident(text, pos)
        if value is None:
            raise _Invalid("an attribute value is expected")
    if _skip_white(text, end) != len(text):
        raise _Invalid("invalid attribute selector")
    return name, op, value


def _parse_selector(text: str):
    """A complex selector -> ([(combinator towards the right neighbour, compound)] rightmost first, specificity)."""
    pos, n, chain, combinator = _skip_white(text, 0), len(text), [], None
    while True:
        comp, pos = _parse_compound(text, pos)
        chain.append((combinator, comp))
        after = _skip_white(text, pos)
        if after == n:
            break
        if text[after] in ">+~":
            combinator, pos = text[after], _skip_white(text, after + 1)
        elif after > pos:
            combinator, pos = " ", after
        else:
            raise _Invalid(f"unexpected {text[after]!r}")
    spec = (0, 0, 0)
    for _c, comp in chain:
        spec = tuple(x + y for x, y in zip(spec, comp.specificity()))
    # stored rightmost first; each entry carries the combinator that joins it to the compound on its right
    out, right = [], None
    for combinator, comp in reversed(chain):
        out.append((right, comp))
        right = combinator
    return out, spec


# ---------------------------------------------------------------------------------------------------------------------
# declarations and rules
# ---------------------------------------------------------------------------------------------------------------------
def parse_declarations(text: str, warn=None) -> tuple:
    """The declarations of a block or of a ``style`` attribute: a tuple of ``(property, value, important)``."""
    warn = warn or (lambda key, message: warnings.warn(message))
    out, pos, n = [], 0, len(text)
    while pos < n:
        end = _scan(text, pos, ";")
        decl, pos = text[pos:end], end + 1
        if not decl.strip():
            continue
        start = _skip_white(decl, 0)
        name, after = _ident(decl, start)
        colon = _skip_white(decl, after)
        if name is None or colon >= len(decl) or decl[colon] != ":":
            warn(("declaration", decl), f"malformed declaration skipped: {decl.strip()[:60]}")
            continue
        value = decl[colon + 1:].strip()
        important = _IMPORTANT.search(value)
        if important is not None:
            value = value[:important.start()].rstrip()
        if not value or _scan(value, 0, "!{}") < len(value):
            warn(("declaration", decl), f"malformed declaration skipped: {decl.strip()[:60]}")
            continue
        out.append((name if name.startswith("--") else name.lower(), value, important is not None))
    return tuple(out)


def _media_applies(prelude: str) -> bool:
    """Whether a media query list is one this loader renders for: an empty query, ``all`` or ``screen`` (``only`` accepted).
    ``not``, other media types and media features never match: the viewport is not known when a document loads."""
    if not prelude.strip():
        return True
    for query in prelude.split(","):
        words = query.lower().split()
        if words[:1] == ["only"]:
            words = words[1:]
        if not words or words in (["all"], ["screen"]):
            return True
    return False


class _Parser:
    def __init__(self, seen):
        self.seen = set() if seen is None else seen   # what has been warned about (shared by the sheets of one document)
        self.rules, self.selectors = [], []

    def warn(self, key, message):
        if key not in self.seen:
            self.seen.add(key)
            warnings.warn(message)

    def rule_list(self, text: str, top: bool):
        pos, n = 0, len(text)
        while True:
            pos = _skip_white(text, pos)
            if pos >= n:
                return
            if top and (text.startswith("<!--", pos) or text.startswith("-->", pos)):
                pos += 4 if text[pos] == "<" else 3
                continue
            if text[pos] == "}":
                self.warn("stray", "stylesheet: a stray } is skipped")
                pos += 1
                continue
            if text[pos] == "@":
                pos = self.at_rule(text, pos)
                continue
            brace = _scan(text, pos, "{}" if not top else "{")
            if brace >= n or text[brace] != "{":
                self.warn(("rule", text[pos:brace]), f"stylesheet: a rule without a block is skipped: {text[pos:brace].strip()[:60]}")
                pos = brace
                continue
            close = _scan(text, brace + 1, "}")
            if close >= n:
                self.warn(("unclosed", text[pos:brace]), f"stylesheet: unclosed block of {text[pos:brace].strip()[:60]!r}: closed at the end of the sheet")
            self.qualified_rule(text[pos:brace].strip(), text[brace + 1:close])
            pos = close + 1

    def at_rule(self, text: str, pos: int) -> int:
        n = len(text)
        name, after = _ident(text, pos + 1)
        name = (name or "").lower()
        end = _scan(text, after, "{;")
        prelude = text[after:end]
        if end >= n or text[end] == ";":   # a statement at-rule
            if name == "import":
                self.warn("import", "@import is not followed: nothing is fetched")
            elif name not in ("charset", "namespace"):
                self.warn(("at", name), f"stylesheet: @{name} is not supported and skipped")
            return end + 1
        close = _scan(text, end + 1, "}")
        if name == "media":
            if _media_applies(prelude):
                self.rule_list(text[end + 1:close], False)
            else:
                self.warn("media", "stylesheet: @media queries with not, another media type or a media feature do not apply (only all and screen do)")
        elif name == "import":
            self.warn("import", "@import is not followed: nothing is fetched")
        elif name not in ("charset", "namespace"):
            kind = name[name.index("-", 1) + 1:] if name.startswith("-") and "-" in name[1:] else name
            self.warn(("at", kind), f"stylesheet: @{kind} is not supported and skipped" if kind in _SKIPPED_AT_RULES
                      else f"stylesheet: unknown at-rule @{name} skipped")
        return close + 1

    def qualified_rule(self, prelude: str, block: str):
        parsed, pos = [], 0
        try:
            if not prelude:
                raise _Invalid("a selector is expected")
            while pos <= len(prelude):
                end = _scan(prelude, pos, ",")
                one = prelude[pos:end].strip()
                if not one:
                    raise _Invalid("an empty selector")
                parsed.append((one, *_parse_selector(one)))
                pos = end + 1
        except _Invalid as e:
            self.warn(("selector", prelude), f"stylesheet: rule dropped, invalid selector {prelude[:80]!r}: {e}")
            return
        declarations = parse_declarations(block, self.warn)
        for one, chain, spec in parsed:
            self.rules.append(Rule(" ".join(one.split()), spec, len(self.rules), declarations))
            self.selectors.append(chain)


def parse_css(text, _seen=None) -> Stylesheet:
    """Style sheet text -> ``Stylesheet``.  Never raises on its input; what is skipped or not understood warns (each kind once)."""
    parser = _Parser(_seen)
    try:
        parser.rule_list(_strip_comments(str(text)), True)
    except RecursionError:
        warnings.warn("stylesheet: nested too deeply: the rest of the sheet is skipped")
    return Stylesheet(parser.rules, parser.selectors)


# ---------------------------------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------------------------------
def _local(name: str) -> str:
    return name.rsplit("}", 1)[-1]


def _attribute(element, name):
    value = element.attrib.get(name)
    if value is None and element.attrib:
        for key, v in element.attrib.items():
            if key[0] == "{" and _local(key) == name:
                return v
    return value


class Matcher:
    """The rules of a sheet against the elements of one document.  ``xml.etree`` has neither parents nor siblings: one walk at
    construction builds a parent map and a child-index map.  The rules are indexed by the id, a class or the type their
    rightmost compound demands (else they go to a short "any element" list), so an element is tested only against rules that can
    match it; a selector is matched right to left."""

    def __init__(self, sheet: Stylesheet, root):
        self.sheet = sheet
        self.parent = {root: None}
        self.index = {root: 0}        # position among the parent's element children
        stack = [root]
        while stack:
            node = stack.pop()
            for i, child in enumerate(node):
                self.parent[child] = node
                self.index[child] = i
                stack.append(child)
        self.by_id, self.by_class, self.by_tag, self.any = {}, {}, {}, []
        for k, chain in enumerate(sheet._selectors):
            comp = chain[0][1]
            if comp.never or comp.elements:
                continue   # (can never match)
            if comp.ids:
                self.by_id.setdefault(comp.ids[0], []).append(k)
            elif comp.classes:
                self.by_class.setdefault(comp.classes[0], []).append(k)
            elif comp.tag is not None:
                self.by_tag.setdefault(comp.tag, []).append(k)
            else:
                self.any.append(k)

    def declarations(self, element) -> list:
        """The declaration tuples of the rules that match `element`, in cascade order: by specificity, then source order."""
        found = list(self.any)
        found += self.by_tag.get(_local(element.tag), ())
        ident = element.attrib.get("id")
        if ident is not None and self.by_id:
            found += self.by_id.get(ident, ())
        classes = element.attrib.get("class")
        if classes and self.by_class:
            for name in set(classes.split()):
                found += self.by_class.get(name, ())
        if not found:
            return []
        rules, selectors = self.sheet.rules, self.sheet._selectors
        hits = [rules[k] for k in found if self.matches(selectors[k], 0, element)]
        hits.sort(key=lambda r: (r.specificity, r.index))
        return [r.declarations for r in hits]

    def matches(self, chain, k, element) -> bool:
        """Whether `element` is what ``chain[k]`` describes, with the rest of the chain found around it."""
        if not self.compound(chain[k][1], element):
            return False
        if k + 1 == len(chain):
            return True
        link = chain[k + 1][0]
        if link == ">":
            parent = self.parent.get(element)
            return parent is not None and self.matches(chain, k + 1, parent)
        if link == " ":
            parent = self.parent.get(element)
            while parent is not None:
                if self.matches(chain, k + 1, parent):
                    return True
                parent = self.parent.get(parent)
            return False
        parent = self.parent.get(element)
        if parent is None:
            return False
        at = self.index[element]
        if link == "+":
            return at > 0 and self.matches(chain, k + 1, parent[at - 1])
        return any(self.matches(chain, k + 1, parent[i]) for i in range(at - 1, -1, -1))   # "~"

    def compound(self, comp: _Compound, element) -> bool:
        if comp.never or comp.elements:
            return False
        if comp.tag is not None and comp.tag != _local(element.tag):
            return False
        attrib = element.attrib
        if comp.ids:
            ident = attrib.get("id")
            if any(i != ident for i in comp.ids):
                return False
        if comp.classes:
            have = (attrib.get("class") or "").split()
            if any(c not in have for c in comp.classes):
                return False
        for name, op, want in comp.attrs:
            value = _attribute(element, name)
            if value is None:
                return False
            if op is None:
                continue
            if op == "=":
                ok = value == want
            elif op == "~=":
                ok = bool(want) and not any(c in want for c in _WHITE) and want in value.split()
            elif op == "|=":
                ok = value == want or value.startswith(want + "-")
            elif op == "^=":
                ok = bool(want) and value.startswith(want)
            elif op == "$=":
                ok = bool(want) and value.endswith(want)
            else:
                ok = bool(want) and want in value
            if not ok:
                return False
        for name, argument in comp.pseudos:
            if not self.pseudo(name, argument, element):
                return False
        return not any(self.compound(inner, element) for inner in comp.nots)

    def pseudo(self, name, argument, element) -> bool:
        parent = self.parent.get(element)
        if name == "root":
            return parent is None
        if parent is None:   # (the root is the only child of the document)
            at, count, same = 0, 1, [element]
        else:
            at, count = self.index[element], len(parent)
            same = None
        if name == "first-child":
            return at == 0
        if name == "last-child":
            return at == count - 1
        if name == "only-child":
            return count == 1
        if name in ("nth-child", "nth-last-child"):
            a, b = argument
            pos = at + 1 if name == "nth-child" else count - at
            return pos == b if a == 0 else (pos - b) % a == 0 and (pos - b) // a >= 0
        if same is None:
            same = [child for child in parent if child.tag == element.tag]
        return same[0] is element if name == "first-of-type" else same[-1] is element
