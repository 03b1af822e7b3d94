"""The device operators report to the host through flag bits in word 0 of ctx->d_status.  Every flag has a name, defined once
per meaning (the common MDB_ST_* set and one prefixed set per operator), and no kernel raises a bare number: a number means
different things to different operators, a name does not."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_NAME = r'(?:[A-Z][A-Z0-9]*_)+ST_[A-Z0-9_]+'


def _sources():
    files = glob.glob(os.path.join(ROOT, "midoridb_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "midoridb_amd", "csrc", "*.h"))
    assert len(files) > 15
    return {os.path.basename(f): open(f).read() for f in files}


def _raise_flag_arguments(text):
    """the second argument of every mdb_raise( call (not of the function's own definition)"""
    out = []
    for m in re.finditer(r'\bmdb_raise\(', text):
        if re.search(r'void\s+$', text[:m.start()]):
            continue
        depth, i, comma = 1, m.end(), None
        while depth:
            c = text[i]
            depth += c == '('
            depth -= c == ')'
            if c == ',' and depth == 1 and comma is None:
                comma = i
            i += 1
        assert comma is not None, text[m.start():i]
        out.append(text[comma + 1:i - 1].strip())
    return out


def test_no_kernel_raises_a_bare_number():
    calls = 0
    for name, text in _sources().items():
        for arg in _raise_flag_arguments(text):
            calls += 1
            assert not re.search(r'\d', re.sub(r'[A-Za-z_]\w*', '', arg)), (name, arg)
    assert calls > 70, calls


def test_every_flag_name_is_used():
    src = _sources()
    defined = {}
    for name, text in src.items():
        for m in re.finditer(r'^#define (%s)\s' % FLAG_NAME, text, re.M):
            assert m.group(1) not in defined, (m.group(1), name, defined[m.group(1)])  # one definition per name
            defined[m.group(1)] = name
    assert len(defined) > 30, sorted(defined)
    whole = "\n".join(src.values())
    whole = re.sub(r'static_assert\(mdb_flags_distinct\(\{.*?\}\)', '', whole, flags=re.S)  # (the sets' own proofs are no use)
    whole = re.sub(r'^#define (%s)\s' % FLAG_NAME, '', whole, flags=re.M)
    used = set(re.findall(r'\b%s\b' % FLAG_NAME, whole))
    assert not sorted(set(defined) - used), sorted(set(defined) - used)
