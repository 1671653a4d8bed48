"""The restatement of emqx_authz_rule (tests/authz_ref.py) against every case transcribed from
the reference's own suites (tests/golden/authz_kats.json)."""

import ipaddress

import pytest

from tests import authz_cases as C
from tests import authz_ref as R

TABLES = C.fixture_tables()
NAME = {R.NOMATCH: "nomatch", R.ALLOW: "allow", R.DENY: "deny", R.BAD: "bad"}


@pytest.mark.parametrize("table", TABLES, ids=[t.name for t in TABLES])
def test_fixture_case(table):
    verdicts, tags = table.reference()
    got = [NAME[v] for v in verdicts]
    for req, g, e in zip(zip(*table.requests), got, table.expect):
        assert g == e, (table.name, req)
    # a deciding rule has a tag, nomatch has none
    for v, t, e in zip(*table.load(R.RefTable()).check(*table.requests), table.expect):
        assert (t == R.TAG_NONE) == (v == R.NOMATCH)


def test_every_quirk_has_a_case():
    names = [t.name for t in TABLES]
    for q in ("Q1", "Q2", "Q3", "Q4", "Q5", "Q6", "Q7"):
        assert any(n.startswith(q + "_") for n in names), q


def test_cidr_vectors():
    for s, lo, hi, n in C.load_kats()["cidr"]:
        assert R.parse_cidr(s) == (int(ipaddress.IPv4Address(lo)), int(ipaddress.IPv4Address(hi)), n)


def test_match_clause_order():
    # match([H | T1], [H | T2]) comes before match(_, ['#']) (emqx_topic.erl:76-81)
    assert R.topic_match(R.words(b"#"), R.words(b"#"))
    assert not R.topic_match(R.words(b"#/x"), R.words(b"#"))
    assert R.topic_match(R.words(b"a"), R.words(b"a/#"))
    assert R.topic_match(R.words(b"$SYS/x"), R.words(b"#"))
