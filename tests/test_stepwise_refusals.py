"""What the ten step-wise entry points of mz_stepwise.hip refuse, and in which order: one table of calls, each a refusal
the library returns before any launch, with the status code and the full text of mzs_last_error.  Shape B = 3, A = 2,
C = 2, E = 4, S = 5; one rooted and one unrooted handle per policy family (MuZero, Gumbel, stochastic).  A case overrides
arguments of an otherwise valid raw call; the `both:` cases violate two conditions at once and pin which one is reported."""
import ctypes as C

import pytest
import torch

from muax_amd import _lib

B, A, CH, E, S = 3, 2, 2, 4, 5

# entry -> its arguments after the handle, in ABI order
ENTRIES = {
    "mzs_root": ["prior_logits", "value", "embedding", "invalid_actions", "dirichlet_noise", "dirichlet_fraction", "key"],
    "mzs_root_gumbel": ["prior_logits", "value", "embedding", "invalid_actions", "gumbel", "key"],
    "mzs_select": ["sim", "action_out", "parent_embedding_out"],
    "mzs_expand_backup": ["sim", "reward", "discount", "prior_logits", "value", "next_embedding"],
    "mzs_expand_backup_select": ["sim", "reward", "discount", "prior_logits", "value", "next_embedding", "next_action_out",
                                 "next_parent_embedding_out"],
    "mzs_finish": ["temperature", "gumbel", "action_out", "action_weights_out", "search_value_out", "depth_sum_out"],
    "mzs_root_stochastic": ["prior_logits", "value", "embedding", "invalid_actions", "dirichlet_noise", "dirichlet_fraction",
                            "key"],
    "mzs_select_stochastic": ["sim", "slot_out", "parent_is_decision_out", "parent_embedding_out"],
    "mzs_expand_backup_stochastic": ["sim", "o"],
    "mzs_finish_stochastic": ["temperature", "gumbel", "action_out", "action_weights_out", "search_value_out",
                              "depth_sum_out"],
}
STOCHASTIC_OUTPUTS = ["chance_logits", "afterstate_value", "afterstate_embedding", "action_logits", "value", "reward",
                      "discount", "state_embedding"]
OPTIONAL = {"invalid_actions", "dirichlet_noise", "gumbel", "search_value_out", "depth_sum_out"}  # null in a valid call
SCALARS = {"sim": 0, "temperature": 1.0, "dirichlet_fraction": 0.0}
NEEDS_SIM = [e for e, names in ENTRIES.items() if "sim" in names]
# the entry's required pointers, under the name its refusal gives them
NULLS = {
    "mzs_root": ("null input", ["prior_logits", "value", "embedding"]),
    "mzs_root_gumbel": ("null input", ["prior_logits", "value", "embedding"]),
    "mzs_select": ("null output", ["action_out", "parent_embedding_out"]),
    "mzs_expand_backup": ("null input", ["reward", "discount", "prior_logits", "value", "next_embedding"]),
    "mzs_expand_backup_select": ("null input", ["reward", "discount", "prior_logits", "value", "next_embedding"]),
    "mzs_finish": ("null output", ["action_out", "action_weights_out"]),
    "mzs_root_stochastic": ("null input", ["prior_logits", "value", "embedding"]),
    "mzs_select_stochastic": ("null output", ["slot_out", "parent_is_decision_out", "parent_embedding_out"]),
    "mzs_expand_backup_stochastic": ("null input", ["o." + f for f in STOCHASTIC_OUTPUTS]),
    "mzs_finish_stochastic": ("null output", ["action_out", "action_weights_out"]),
}
DETERMINISTIC = ["mzs_root", "mzs_root_gumbel", "mzs_select", "mzs_expand_backup", "mzs_expand_backup_select", "mzs_finish"]
STOCHASTIC = ["mzs_root_stochastic", "mzs_select_stochastic", "mzs_expand_backup_stochastic", "mzs_finish_stochastic"]


def _table():
    """(case id, handle, entry, overrides, expected text after "<entry>: ")"""
    t = []
    add = lambda what, handle, entry, over, text: t.append((f"{entry}-{what}", handle, entry, over, text))  # noqa: E731
    # a handle of the other family
    add("stochastic_handle", "stochastic", "mzs_root", {}, "this handle runs the stochastic policy; use mzs_root_stochastic")
    add("gumbel_handle", "gumbel", "mzs_root", {}, "this handle runs the gumbel policy; use mzs_root_gumbel")
    add("muzero_handle", "muzero", "mzs_root_gumbel", {}, "this handle does not run the gumbel policy (policy 1)")
    add("stochastic_handle", "stochastic", "mzs_root_gumbel", {}, "this handle does not run the gumbel policy (policy 1)")
    for e, use in (("mzs_select", "mzs_select_stochastic"), ("mzs_expand_backup", "mzs_expand_backup_stochastic"),
                   ("mzs_expand_backup_select", "mzs_expand_backup_stochastic"), ("mzs_finish", "mzs_finish_stochastic")):
        add("stochastic_handle", "stochastic", e, {}, f"this handle runs the stochastic policy; use {use}")
    for e in STOCHASTIC:
        for fam in ("muzero", "gumbel"):
            add(f"{fam}_handle", fam, e, {}, "this handle does not run the stochastic policy (policy 2)")
    # a call before the root
    for e in DETERMINISTIC[2:]:
        for fam in ("muzero0", "gumbel0"):
            add(f"before_root_{fam[:-1]}", fam, e, {}, "call mzs_root first")
    for e in STOCHASTIC[1:]:
        add("before_root", "stochastic0", e, {}, "call mzs_root_stochastic first")
    # sim out of range
    for e in NEEDS_SIM:
        for sim in (-1, S):
            add(f"sim_{sim}", "stochastic" if e in STOCHASTIC else "muzero", e, {"sim": sim}, "sim out of range")
    # each null pointer
    for e, (text, names) in NULLS.items():
        for n in names:
            add(f"null_{n}", "stochastic" if e in STOCHASTIC else ("gumbel" if e == "mzs_root_gumbel" else "muzero"), e,
                {n: None}, text)
    for n in ("next_action_out", "next_parent_embedding_out"):
        add(f"null_{n}", "muzero", "mzs_expand_backup_select", {n: None}, "null output")
    add("null_o", "stochastic", "mzs_expand_backup_stochastic", {"o": None}, "null or size mismatch (ABI)")
    add("struct_size", "stochastic", "mzs_expand_backup_stochastic", {"o.struct_size": 8}, "null or size mismatch (ABI)")
    # noise fraction without noise
    for e, fam in (("mzs_root", "muzero"), ("mzs_root", "muzero0"), ("mzs_root_stochastic", "stochastic")):
        add(f"fraction_without_noise_{fam}", fam, e, {"dirichlet_fraction": 0.25}, "dirichlet_fraction != 0 needs dirichlet_noise")
    # two violations at once: the deterministic family ...
    add("both:null_input+stochastic_handle", "stochastic", "mzs_root", {"value": None}, "null input")
    add("both:fraction+gumbel_handle", "gumbel", "mzs_root", {"dirichlet_fraction": 0.25},
        "dirichlet_fraction != 0 needs dirichlet_noise")
    add("both:null_input+fraction", "muzero", "mzs_root", {"embedding": None, "dirichlet_fraction": 0.25}, "null input")
    add("both:null_input+muzero_handle", "muzero", "mzs_root_gumbel", {"prior_logits": None}, "null input")
    add("both:before_root+stochastic_handle", "stochastic0", "mzs_select", {}, "call mzs_root first")
    add("both:sim+stochastic_handle", "stochastic", "mzs_select", {"sim": -1}, "sim out of range")
    add("both:null_output+stochastic_handle", "stochastic", "mzs_select", {"action_out": None}, "null output")
    add("both:before_root+sim", "muzero0", "mzs_select", {"sim": S}, "call mzs_root first")
    add("both:sim+null_input", "muzero", "mzs_expand_backup", {"sim": S, "reward": None}, "sim out of range")
    add("both:null_input+stochastic_handle", "stochastic", "mzs_expand_backup", {"value": None}, "null input")
    add("both:null_output+before_root", "gumbel0", "mzs_expand_backup_select", {"next_action_out": None}, "null output")
    add("both:null_output+sim", "muzero", "mzs_expand_backup_select", {"next_parent_embedding_out": None, "sim": -1},
        "null output")
    add("both:before_root+null_input", "muzero0", "mzs_expand_backup_select", {"discount": None}, "call mzs_root first")
    add("both:before_root+null_output", "muzero0", "mzs_finish", {"action_out": None}, "call mzs_root first")
    add("both:null_output+stochastic_handle", "stochastic", "mzs_finish", {"action_weights_out": None}, "null output")
    # ... and the stochastic one
    add("both:muzero_handle+null_input", "muzero", "mzs_root_stochastic", {"prior_logits": None},
        "this handle does not run the stochastic policy (policy 2)")
    add("both:gumbel_handle+fraction", "gumbel", "mzs_root_stochastic", {"dirichlet_fraction": 0.25},
        "this handle does not run the stochastic policy (policy 2)")
    add("both:null_input+fraction", "stochastic", "mzs_root_stochastic", {"value": None, "dirichlet_fraction": 0.25},
        "null input")
    add("both:muzero_handle+sim", "muzero", "mzs_select_stochastic", {"sim": -1},
        "this handle does not run the stochastic policy (policy 2)")
    add("both:before_root+sim", "stochastic0", "mzs_select_stochastic", {"sim": S}, "call mzs_root_stochastic first")
    add("both:sim+null_output", "stochastic", "mzs_select_stochastic", {"sim": S, "slot_out": None}, "sim out of range")
    add("both:before_root+struct_size", "stochastic0", "mzs_expand_backup_stochastic", {"o.struct_size": 8},
        "call mzs_root_stochastic first")
    add("both:sim+null_o", "stochastic", "mzs_expand_backup_stochastic", {"sim": -1, "o": None}, "sim out of range")
    add("both:struct_size+null_input", "stochastic", "mzs_expand_backup_stochastic", {"o.struct_size": 8, "o.reward": None},
        "null or size mismatch (ABI)")
    add("both:gumbel_handle+null_output", "gumbel", "mzs_finish_stochastic", {"action_out": None},
        "this handle does not run the stochastic policy (policy 2)")
    add("both:before_root+null_output", "stochastic0", "mzs_finish_stochastic", {"action_out": None},
        "call mzs_root_stochastic first")
    return t


TABLE = _table()


def _call(L, handle, entry, over, buf):
    """The raw call of `entry` with valid arguments but for `over` (a name -> value; "o.<field>": a member of the struct)."""
    keep, args = [], []
    for n in ENTRIES[entry]:
        if n == "o":
            o = _lib.args(_lib.MzsStochasticOutputs, **{f: buf.data_ptr() for f in STOCHASTIC_OUTPUTS})
            for k, v in over.items():
                if k.startswith("o."):
                    setattr(o, k[2:], v)
            keep.append(o)
            v = C.byref(o)
        elif n == "key":
            keep.append((C.c_uint32 * 2)(1, 2))
            v = C.byref(keep[-1])
        elif n in SCALARS:
            v = SCALARS[n]
        else:
            v = None if n in OPTIONAL else C.c_void_p(buf.data_ptr())
        if n in over:
            v = over[n]
        if n in ("temperature", "dirichlet_fraction"):
            v = C.c_float(v)
        args.append(v)
    return getattr(L, entry)(handle, *args, None)


@pytest.fixture(scope="module")
def handles():
    """muzero / gumbel / stochastic: rooted; muzero0 / gumbel0 / stochastic0: never rooted."""
    from muax_amd import MuZeroSearch, SearchConfig
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    cfgs = {"muzero": SearchConfig(A, S, E), "gumbel": SearchConfig(A, S, E, policy="gumbel", tiebreak=False),
            "stochastic": SearchConfig(A, S, E, policy="stochastic", num_chance_outcomes=CH)}
    hs = {}
    for fam, cfg in cfgs.items():
        hs[fam], hs[fam + "0"] = MuZeroSearch(B, cfg), MuZeroSearch(B, cfg)
    hs["muzero"].root(z(B, A), z(B), z(B, E))
    hs["gumbel"].root_gumbel(z(B, A), z(B), z(B, E))
    hs["stochastic"].root_stochastic(z(B, A), z(B), z(B, E))
    hs["buf"] = z(64)  # what every valid pointer points to (no refused call reads or writes it)
    torch.cuda.synchronize()
    yield hs
    for k, h in hs.items():
        if k != "buf":
            h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("handle,entry,over,text", [pytest.param(*c[1:], id=c[0]) for c in TABLE])
def test_refusal_status_and_text(handles, handle, entry, over, text):
    L = _lib.load()
    h = handles[handle]
    assert _call(L, h._h, entry, over, handles["buf"]) == _lib.MZS_E_INVALID
    assert L.mzs_last_error(h._h).decode() == f"{entry}: {text}"


@pytest.mark.gpu
def test_wrappers_raise_the_refusal(handles):
    """The same refusals through MuZeroSearch's methods (one per entry): ValueError with the library's text."""
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    d, g, s = handles["muzero"], handles["gumbel0"], handles["stochastic"]
    rec = (z(B), z(B), z(B, A), z(B), z(B, E))
    sto = ((z(B, CH), z(B)), z(B, E), (z(B, A), z(B), z(B), z(B)), z(B, E))
    for call, text in [
            (lambda: s.root(z(B, A), z(B), z(B, E)), "mzs_root: this handle runs the stochastic policy; use mzs_root_stochastic"),
            (lambda: d.root_gumbel(z(B, A), z(B), z(B, E)), "mzs_root_gumbel: this handle does not run the gumbel policy (policy 1)"),
            (lambda: d.select(S), "mzs_select: sim out of range"),
            (lambda: d.expand_backup(-1, *rec), "mzs_expand_backup: sim out of range"),
            (lambda: d.expand_backup_select(S, *rec), "mzs_expand_backup_select: sim out of range"),
            (lambda: g.finish(), "mzs_finish: call mzs_root first"),
            (lambda: d.root_stochastic(z(B, A), z(B), z(B, E)),
             "mzs_root_stochastic: this handle does not run the stochastic policy (policy 2)"),
            (lambda: s.select_stochastic(-1), "mzs_select_stochastic: sim out of range"),
            (lambda: s.expand_backup_stochastic(S, *sto), "mzs_expand_backup_stochastic: sim out of range"),
            (lambda: d.finish_stochastic(), "mzs_finish_stochastic: this handle does not run the stochastic policy (policy 2)")]:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_null_handle_is_refused_by_every_entry():
    """No handle, no text: MZS_E_INVALID (host code alone, no device needed)."""
    L = _lib.load()
    buf = torch.zeros(64)
    for entry in ENTRIES:
        assert _call(L, None, entry, {}, buf) == _lib.MZS_E_INVALID, entry
