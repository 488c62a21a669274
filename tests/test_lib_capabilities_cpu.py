"""_lib.load / _lib.capabilities against stand-in libraries (no GPU, nothing dlopened): which entry points get prototypes and which
features are reported for an older PRIMX_LIB A/B build, for a version-35 build from before an entry point that joined it without a new
number, and for the current build; an unknown version is refused and a missing declared symbol is an AttributeError."""
import pytest

from topia_xl_amd import _lib

ALL = frozenset({"fold", "blocks_call", "kv_ride", "f32out_group", "null_skip", "attn_ksplit", "toq64"})
# the entry points that joined version 35 without a new number (include/primx_hip.h)
UNNUMBERED = {"primx_material_sample", "primx_attention_ksplit_mode", "primx_attention_ksplit", "primx_gemm_toq64_mode",
              "primx_dit_blocks_fold_features"}


class StandIn:
    """Looks like a ctypes.CDLL to _lib.load: the symbols in `names` are attributes (plain functions, so prototypes can be attached)."""

    def __init__(self, version, names, features=1):
        self._fns = {}
        for name in names:
            self._fns[name] = self._make({"primx_abi_version": version, "primx_dit_blocks_fold_features": features}.get(name, 0))

    @staticmethod
    def _make(value):
        def fn(*args):
            return value
        return fn

    def __getattr__(self, name):
        try:
            return self.__dict__["_fns"][name]
        except KeyError:
            raise AttributeError(name) from None

    def bound(self):
        return {name for name, fn in self._fns.items() if hasattr(fn, "argtypes")}


def _load(monkeypatch, tmp_path, lib, ab=True):
    path = str(tmp_path / "libstandin.so")
    open(path, "wb").close()
    monkeypatch.setattr(_lib, "_caps", {})
    monkeypatch.setattr(_lib.C, "CDLL", lambda p: lib)
    if ab:
        monkeypatch.setenv("PRIMX_LIB", path)
    else:
        monkeypatch.delenv("PRIMX_LIB", raising=False)
    assert _lib.load(path) is lib
    return _lib.capabilities(path)


def _since(name):
    return _lib._SINCE.get(name, 21)


def test_the_table_names_declared_entry_points_only():
    assert set(_lib._SINCE) <= set(_lib.SIGNATURES) and set(_lib._FEATURES.values()) <= set(_lib.SIGNATURES)
    assert {n for n, v in _lib._SINCE.items() if v == _lib._PROBE} == UNNUMBERED
    assert all(v == _lib._PROBE or 21 < v <= _lib.ABI_VERSION for v in _lib._SINCE.values())
    assert set(_lib._FEATURES) == ALL


@pytest.mark.parametrize("version, caps", [(22, set()), (24, {"fold", "blocks_call"}), (25, {"fold", "blocks_call", "kv_ride"}),
                                           (34, {"fold", "blocks_call", "kv_ride", "f32out_group"})])
def test_an_older_ab_build_binds_what_its_version_has(monkeypatch, tmp_path, version, caps):
    # the build carries every symbol of its version - and, before 23, fold entry points with OTHER argument lists, which must stay unbound
    names = {n for n in _lib.SIGNATURES if n not in UNNUMBERED and (_since(n) <= version or _since(n) == 23)}
    lib = StandIn(version, names)
    assert _load(monkeypatch, tmp_path, lib) == caps
    assert lib.bound() == {n for n in _lib.SIGNATURES if n not in UNNUMBERED and _since(n) <= version}
    assert ("primx_linear_fold" in lib.bound()) == (version >= 23) and ("primx_dit_blocks_fold" in lib.bound()) == (version >= 24)
    assert "primx_linear" in lib.bound() and "primx_raymarch_backward" not in lib.bound()
    assert lib.primx_last_error.restype is _lib.C.c_char_p and lib.primx_linear.restype is _lib.C.c_int
    assert lib.primx_linear.argtypes == _lib.SIGNATURES["primx_linear"]


def test_a_version_35_build_from_before_the_key_split(monkeypatch, tmp_path):
    lib = StandIn(35, set(_lib.SIGNATURES) - {"primx_attention_ksplit", "primx_attention_ksplit_mode"})
    assert _load(monkeypatch, tmp_path, lib) == ALL - {"attn_ksplit"}
    assert lib.bound() == set(lib._fns)
    # ... and, not named by PRIMX_LIB, the same build is refused: a declared symbol is missing
    with pytest.raises(AttributeError):
        _load(monkeypatch, tmp_path, lib, ab=False)


def test_the_null_skip_is_told_by_the_features_word(monkeypatch, tmp_path):
    assert _load(monkeypatch, tmp_path, StandIn(35, set(_lib.SIGNATURES), features=0)) == ALL - {"null_skip"}
    assert _load(monkeypatch, tmp_path, StandIn(35, set(_lib.SIGNATURES) - {"primx_dit_blocks_fold_features"})) == ALL - {"null_skip"}


def test_the_current_build(monkeypatch, tmp_path):
    lib = StandIn(_lib.ABI_VERSION, set(_lib.SIGNATURES))
    assert _load(monkeypatch, tmp_path, lib, ab=False) == ALL
    assert lib.bound() == set(_lib.SIGNATURES)
    for name in ALL:
        monkeypatch.setitem(_lib._caps, _lib.LIB_PATH, frozenset({name}))
        assert [f for f in sorted(ALL) if getattr(_lib, f + "_available")()] == [name]


@pytest.mark.parametrize("version, ab", [(20, True), (36, True), (34, False), (36, False)])
def test_an_unknown_version_is_refused(monkeypatch, tmp_path, version, ab):
    with pytest.raises(RuntimeError, match="ABI"):
        _load(monkeypatch, tmp_path, StandIn(version, set(_lib.SIGNATURES)), ab=ab)
