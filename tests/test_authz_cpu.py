"""CPU-side checks of the authorization table (include/emqx_authz.h) on a host-only handle:
the exports, the rejected inputs, emqx_authz_check_host against the restatement
(tests/authz_ref.py) verdict for verdict and tag for tag, and no batch call without a device."""

import os
import re
import subprocess

import numpy as np
import pytest

from tests import authz_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    lib_path = os.path.join(ROOT, "emqx_amd", "_build", "libemqxmatch.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    from emqx_amd import authz
    return authz


def test_exports_every_authz_symbol(A):
    from emqx_amd import _lib
    from tests.test_abi_cpu import header_functions
    declared = header_functions("emqx_authz.h")
    assert len(declared) >= 12
    assert sorted(_lib.AUTHZ_EXPORTS) == declared
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in declared:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\bT %s\b" % name, nm), name


def check_table(A, table):
    a = table.load(A.Authz(A.HOST_ONLY))
    a.commit()
    verdict, tag = a.check_host(*table.requests, no_match=table.no_match)
    ev, et = table.reference()
    assert verdict.tolist() == ev, table.name
    assert tag.tolist() == et, table.name
    return a


FIXTURE = C.fixture_tables()


@pytest.mark.parametrize("table", FIXTURE, ids=[t.name for t in FIXTURE])
def test_check_host_fixture(A, table):
    check_table(A, table)


@pytest.mark.parametrize("seed", range(20))
def test_check_host_dense_fuzz(A, seed):
    check_table(A, C.dense_table(seed))


@pytest.mark.parametrize("seed", range(3))
def test_check_host_long_fuzz(A, seed):
    a = check_table(A, C.long_table(seed))
    s = a.stats()
    assert s["n_rules"] == 300 and s["n_sources"] == 2 and s["n_lists"] == 4 and s["epoch"] == 1
    assert s["last_evals"] > 0


REJECTED = [
    ("ipv6", [("allow", ("ipaddr", "::1/128"), "all", ["#"])], "IPv6"),
    ("ipv6_in_list", [("allow", ("ipaddrs", ["10.0.0.1", "fe80::/10"]), "all", ["#"])], "IPv6"),
    ("bad_cidr", [("allow", ("ipaddr", "10.0.0.1/33"), "all", ["#"])], "CIDR"),
    ("permission", [("accept", "all", "publish", ["t"])], "permission"),
    ("action", [("allow", "all", "pub", ["t"])], "action"),
    ("long_filter", [("allow", "all", "all", ["a" * 65536])], "65535"),
    ("long_principal", [("allow", ("username", "u" * 65536), "all", ["#"])], "65535"),
    ("flag_bit", [("allow", ("flag", 64), "all", ["#"])], "63"),
]


@pytest.mark.parametrize("name,rules,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_inputs_leave_the_table_unchanged(A, name, rules, word):
    from emqx_amd import _lib
    a = A.Authz(A.HOST_ONLY)
    a.set_list(0, [("deny", "all", "publish", ["keep"])], tags=[7])
    a.set_clients([{"id": 0, "clientid": "c"}])
    # the bad rule comes second: nothing of the call may be stored
    with pytest.raises(_lib.EngineError) as e:
        a.set_list(0, [("allow", "all")] + rules)
    assert e.value.code == _lib.EMQX_EINVAL
    assert word in str(e.value), str(e.value)
    a.commit()
    v, t = a.check_host([0, 0], [1, 1], [b"keep", b"other"])
    assert v.tolist() == [A.DENY, A.NOMATCH] and t.tolist() == [7, A.TAG_NONE]
    assert a.stats()["n_rules"] == 1


def test_nested_who_is_rejected(A):
    a = A.Authz(A.HOST_ONLY)
    with pytest.raises(ValueError):
        a.set_list(0, [("allow", ("and", [("or", [("username", "u")])]), "all", ["#"])])
    # the C ABI has no encoding for nesting: a leaf kind outside the enumeration is refused
    import ctypes
    from emqx_amd import _lib
    from emqx_amd.engine import _ptr, pack
    rule = (_lib.AuthzRule * 1)(_lib.AuthzRule(1, 3, 2, 0, 1, 0, 1, 0))
    who = (_lib.AuthzWho * 1)(_lib.AuthzWho(2 + 3, 0, 0))
    buf, offs = pack([b"#"])
    err = ctypes.create_string_buffer(128)
    rc = _lib.lib().emqx_authz_list_set(a._h, 0, 0, None, 0, rule, 1, who, 1, _ptr(buf), _ptr(offs), 1, err, 128)
    assert rc == _lib.EMQX_EINVAL and b"nest" in err.value


def test_long_client_fields_are_rejected(A):
    from emqx_amd import _lib
    a = A.Authz(A.HOST_ONLY)
    with pytest.raises(_lib.EngineError) as e:
        a.set_clients([{"id": 0, "clientid": "ok"}, {"id": 1, "clientid": "c" * 65536}])
    assert e.value.code == _lib.EMQX_EINVAL
    a.commit()
    assert a.check_host([0], [1], [b"t"])[0].tolist() == [A.BAD_REQUEST]
    assert a.stats()["n_clients"] == 0


def test_commit_publishes_and_drop_forgets(A):
    a = A.Authz(A.HOST_ONLY)
    a.set_list(0, [("allow", "all")])
    a.set_clients([{"id": 5, "clientid": "c"}])
    assert a.check_host([5], [1], [b"t"])[0].tolist() == [A.BAD_REQUEST]  # not committed yet
    a.commit()
    assert a.check_host([5, 4, 6], [1, 1, 1], [b"t"] * 3)[0].tolist() == [A.ALLOW, A.BAD_REQUEST, A.BAD_REQUEST]
    a.drop_clients([5])
    a.set_list(0, [])
    assert a.check_host([5], [2], [b"t"])[0].tolist() == [A.ALLOW]  # the committed snapshot stands
    a.commit()
    assert a.check_host([5], [2], [b"t"])[0].tolist() == [A.BAD_REQUEST]
    assert a.stats()["epoch"] == 2


def test_maximal_lengths(A):
    a = A.Authz(A.HOST_ONLY)
    big = b"x" * 65535
    a.set_list(0, [("allow", ("clientid", big), "all", [b"p/${clientid}", ("eq", big)])])
    a.set_clients([{"id": 0, "clientid": big}, {"id": 1, "clientid": big[:-1]}])
    a.commit()
    v, _ = a.check_host([0, 0, 0, 1], [1, 1, 1, 1], [b"p/" + big, big, big[:-1], big])
    assert v.tolist() == [A.ALLOW, A.ALLOW, A.NOMATCH, A.NOMATCH]


def test_decreasing_offsets_are_einval(A):
    from emqx_amd import _lib
    a = A.Authz(A.HOST_ONLY)
    a.commit()
    with pytest.raises(_lib.EngineError) as e:
        a._run(_lib.lib().emqx_authz_check_host, "check_host", [0, 0], [1, 1], np.zeros(8, np.uint8),
               np.array([0, 4, 2], np.uint64), None)
    assert e.value.code == _lib.EMQX_EINVAL


def test_batch_calls_need_a_device(A):
    from emqx_amd import _lib
    a = A.Authz(A.HOST_ONLY)
    a.set_list(0, [("allow", "all")])
    a.set_clients([{"id": 0}])
    a.commit()
    for call in (lambda: a.check([0], [1], [b"t"]),
                 lambda: a.check_device(0, 0, 0, 0, 0, 0),
                 lambda: a.check_device_async(0, 0, 0, 0, 0, 0, 0, 8)):
        with pytest.raises(_lib.EngineError) as e:
            call()
        assert e.value.code == _lib.EMQX_EDEVICE
