"""Every environment variable the native library reads is documented: the getenv("DCUE_...") names
under csrc/ are exactly the rows of INTEGRATION.md's "Environment variables" table. A knob added
without a row, or a row whose knob was deleted, fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd", "csrc")


def _read_in_csrc():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        with open(path, encoding="utf-8") as fh:
            names |= set(re.findall(r'getenv\("(DCUE_[A-Z0-9_]+)"', fh.read()))
    return names


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = text.split("### Environment variables", 1)[1].split("\n## ", 1)[0]
    rows = re.findall(r"^\| `(DCUE_[A-Z0-9_]+)` \|(.*)\|$", section, flags=re.M)
    for name, rest in rows:  # values, default, purpose, exercised by: none left empty
        cells = [c.strip() for c in rest.split("|")]
        assert len(cells) == 4 and all(cells), name
    names = [name for name, _ in rows]
    assert len(names) == len(set(names)), "a variable is listed twice"
    return set(names)


def test_every_env_knob_is_documented():
    read, doc = _read_in_csrc(), _documented()
    assert read, "no getenv found: the sources moved?"
    assert read - doc == set(), "read by csrc/ but not in INTEGRATION.md: %s" % sorted(read - doc)
    assert doc - read == set(), "in INTEGRATION.md but no longer read: %s" % sorted(doc - read)
