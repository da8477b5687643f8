"""The environment switches of libsr3hip.so, held together as text: every "SR3_..." string literal in csrc/ is a name in
the comment block at the head of csrc/sr3_internal.h and the other way round, INTEGRATION.md and DESIGN.md §7b name each
of them, and each form that a tuned gate guards has both its SR3_NO_<FORM> and its SR3_<FORM>_FORCE switch. Reads the
project's own sources only: no library, no GPU."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "3d-super-resolution-face-reconstruction_amd" / "csrc"
FORMS = ("WINO_GEMM_OUT", "WINO_FUSED_ROWS", "UP2_WINO", "GN_RES1X1")


def literals():
    """every "SR3_[A-Z0-9_]+" string literal of the sources and headers in csrc/"""
    found = set()
    for path in sorted(CSRC.iterdir()):
        if path.suffix in (".hip", ".h", ".cpp"):
            found.update(re.findall(r'"(SR3_[A-Z0-9_]+)"', path.read_text()))
    return found


def documented():
    """the names the comment block at the head of sr3_internal.h describes: its `//   SR3_NAME=value` lines"""
    text = (CSRC / "sr3_internal.h").read_text()
    head = text[text.index("\n", text.index("---- environment switches")) + 1:]
    block = head[:re.search(r"^(?!//)", head, re.M).start()]       # up to the first line that is no comment
    return set(re.findall(r"^//   (SR3_[A-Z0-9_]+)=", block, re.M))


def test_literals_equal_the_documented_names():
    lit, doc = literals(), documented()
    assert lit and doc
    assert lit == doc, f"read but not described: {sorted(lit - doc)}; described but not read: {sorted(doc - lit)}"


def test_integration_names_every_switch():
    text = (ROOT / "INTEGRATION.md").read_text()
    missing = [n for n in sorted(documented()) if not re.search(r"\b%s\b" % n, text)]
    assert not missing, missing


def test_design_7b_names_every_switch_and_counts_them():
    text = (ROOT / "DESIGN.md").read_text()
    sec = text[text.index("## 7b. Switches"):]
    sec = sec[:sec.index("\n## ", 1)]
    missing = [n for n in sorted(documented()) if not re.search(r"\b%s\b" % n, sec)]
    assert not missing, missing
    words = ("zero one two three four five six seven eight nine ten eleven twelve thirteen fourteen fifteen sixteen seventeen "
             "eighteen nineteen twenty").split()
    count = re.match(r"## 7b\. Switches \((\w+) in the library", sec)
    assert count and count.group(1) == words[len(documented())], (count and count.group(1), len(documented()))


def test_each_form_has_its_off_and_its_force_switch():
    names = literals()
    for form in FORMS:
        assert f"SR3_NO_{form}" in names and f"SR3_{form}_FORCE" in names, form
    # and no other pair exists that the list above forgot
    forced = {m.group(1) for n in names if (m := re.fullmatch(r"SR3_([A-Z0-9_]+)_FORCE", n))}
    assert forced == set(FORMS), sorted(forced)
