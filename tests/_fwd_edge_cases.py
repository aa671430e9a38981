"""The case table of the forward tile-edge tests (tests/test_hip_fwd_edges.py runs it on the GPU,
tests/test_fwd_edge_cases_cpu.py checks it without one).  Nothing here touches a GPU or imports the HIP package.

A case is a tests._attention_fp64.Case (so tests._attention_fp64.problem / torch_draws and the shared forward oracle take
it as it is) with five more columns:

  form         the kernel form the case is meant to run (expected_form() derives the same from the dispatch conditions):
                 stream4   acattn_fwd_stream_kernel<DH, 4, ..>, L <= 64          stream13  <DH, 13, ..>, 64 < L <= 208
                 dma       acattn_fwd_dma_kernel, 48 < L <= 64                   fast      acattn_fwd_fast_kernel, L <= 48
                 general   acattn_fwd_general_kernel                             long      the long form, pinned
  fpin         the forward pin (acattn_select_forward_kernel): auto | stream | staged | general | long
  extras       the producer extras (acattn_problem.affine and gate probabilities) are handed over
  adversarial  True = the full operator; False = the spatial-only flavour (one soft-max, one context)
  seed         of the inputs (tests/_attention_fp64.problem)

kind "train" = counter RNG (the oracle is fed the kernel's own draws); kind "general" = explicit randomness
(tests/_attention_fp64.torch_draws on both sides), which only the general kernel takes.  B = 4, two heads; the four
sequences are tests/_attention_fwd_ref.edge_key_valid's.

Lengths: the smallest at which each form can go wrong -- on, one short of and one past a 16-row tile edge, the 64-key
group edges of the 13-tile form (NG: 128 / 129, 192 / 193), both ends of each form's range, lengths that are no multiple of
four (a 16-byte gate or M access then straddles a row end), the tail block (1 <= L % 16 <= 4) at one, two, three and four
rows and one past it (L % 16 = 5).  Head size 32 runs at every length; 16, 64 and 128 at an on-edge, a one-past and a
tail-block length per form, in every (ADV, HALF, PRE) instantiation of the streaming kernels."""
from collections import namedtuple

from tests import _attention_fp64 as F

EdgeCase = namedtuple("EdgeCase", F.Case._fields + ("form", "fpin", "extras", "adversarial", "seed"))

B, NH = 4, 2
FORMS = ("stream4", "stream13", "dma", "fast", "general", "long")
STREAM4_L = (1, 2, 15, 16, 17, 20, 21, 31, 32, 33, 36, 47, 48, 49, 51, 52, 53, 63, 64)
STREAM13_L = (65, 68, 69, 79, 80, 81, 127, 128, 129, 191, 192, 193, 207, 208)
DMA_L = (49, 51, 52, 53, 63, 64)
FAST_L = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48)
GENERAL_L = (1, 15, 16, 17, 49, 64, 65, 193, 208)
LONG_L = (1, 16, 17, 64, 65, 208)
LENGTHS = {"stream4": STREAM4_L, "stream13": STREAM13_L, "dma": DMA_L, "fast": FAST_L, "general": GENERAL_L, "long": LONG_L}
STAGED_HEAD_SIZES = (16, 32, 64)  # launch_dma / launch_fast have no head size 128: that falls through to the general kernel


def tail_block(c):
    """acattn_fwd_stream.inc, acattn_fwd_stream_kernel: `if constexpr (PRE && NT == 4)` ... `if (qb == nT - 1 && (L & 15) != 0
    && (L & 15) <= 4)` -> stream_tail_block.  The last query block of a 4-tile streaming launch with the producer extras
    takes it whatever the mask is and also when it is the only block (L <= 4)."""
    return c.form == "stream4" and c.extras and 1 <= c.L % 16 <= 4


def reordered_grid(c):
    """The same file one statement earlier: `if (PRE && NT == 4 && causal && nT >= 2 && (L & 15) != 0 && (L & 15) <= 4 &&
    rank < 2) qb = nT - 2 + rank;` -- under the causal mask the tail block swaps places with the block in front of it."""
    return tail_block(c) and c.causal and (c.L + 15) // 16 >= 2


def _tuned(c):
    """What acattn_launch_fwd_stream, acattn_launch_fwd_dma and acattn_launch_fwd_fast all ask of a problem (`ok`):
    structured mask, counter RNG, both spatial terms, and with the adversarial calibrator `gate` and two_level."""
    return (c.mask == "structured" and c.kind == "train" and set(c.terms) == {"order", "distance"}
            and (not c.adversarial or (c.combine == "gate" and c.two_level)))


def expected_form(c):
    """acattn_fwd.hip::acattn_launch_fwd, top to bottom."""
    dh = c.H // c.nh
    # `if (which == ACATTN_FWD_LONG || (which == ACATTN_FWD_AUTO && p.L > 208)) return acattn_launch_fwd_long(..)`
    if c.fpin == "long" or (c.fpin == "auto" and c.L > 208):
        return "long"
    assert c.L <= 208  # (a pinned kernel above 208 keys is an error)
    if c.fpin != "general":  # `if (which != ACATTN_FWD_GENERAL)`
        if c.fpin in ("auto", "stream") and _tuned(c) and dh in (16, 32, 64, 128):
            # acattn_launch_fwd_stream: `pre = p.affine && (gate_prob || !p.adversarial)`; `if (gate_prob && !pre) return -100`
            # (extras here always means both the planes and the probabilities, so that refusal does not arise);
            # acattn_launch_fwd_stream_dh*: `if (p.L <= 64)` -> launch_stream_nt<DH, 4, PRE>, else <DH, 13, PRE>
            return "stream4" if c.L <= 64 else "stream13"
        # acattn_launch_fwd_dma: `p.L > 48 && p.L <= 64`, head sizes 16 / 32 / 64
        if _tuned(c) and 48 < c.L <= 64 and dh in STAGED_HEAD_SIZES:
            return "dma"
        # acattn_launch_fwd_fast: `p.L <= 64` (reached only at L <= 48), head sizes 16 / 32 / 64
        if _tuned(c) and c.L <= 64 and dh in STAGED_HEAD_SIZES:
            return "fast"
    return "general"


def instantiation(c):
    """The template arguments the launch functions pick: launch_stream_nt (`half = p.p_drop == 0.5f`, p.adversarial, PRE),
    launch_dma / launch_fast (<DH, ADV>); the general and the long kernels are <DH, ..> with run-time options."""
    dh = c.H // c.nh
    if c.form in ("stream4", "stream13"):
        return (c.form, dh, c.adversarial, c.p_drop == 0.5, c.extras)
    return (c.form, dh, c.adversarial)


def _table():
    cases, seen = [], set()

    def add(form, fpin, L, dh=32, causal=True, p=0.5, extras=False, adv=True, kind="train", tag="", seed=606, **kw):
        cid = (f"{form}-{fpin}-L{L}-dh{dh}-{'causal' if causal else 'bidir'}-p{p}-{'extras' if extras else 'plain'}-"
               f"{'adv' if adv else 'spatial'}" + (f"-{tag}" if tag else ""))
        if cid in seen:
            return
        seen.add(cid)
        base = F._case(cid, kind, (B, L, NH * dh, NH), causal=causal, p_drop=p, **kw)
        cases.append(EdgeCase(*base, form, fpin, extras, adv, seed))

    # ---- streaming, head size 32, every length ----------------------------------------------------------------------------
    for form, lengths in (("stream4", STREAM4_L), ("stream13", STREAM13_L)):
        for n, L in enumerate(lengths):
            add(form, "stream", L, extras=True)
            add(form, "stream", L, extras=False)
            add(form, "stream", L, causal=False, p=0.1, extras=n % 2 == 0)
            add(form, "stream", L, causal=n % 2 == 1, p=0.0, extras=n % 2 == 1, adv=False)
            if form == "stream4" and 1 <= L % 16 <= 4:
                # the tail lengths under the other mask and without the extras (the ordinary path), and the tail block's
                # other instantiations
                add(form, "stream", L, causal=False, extras=False)
                add(form, "stream", L, causal=False, extras=True)
                add(form, "stream", L, p=0.1, extras=True)
                add(form, "stream", L, p=0.1, extras=True, adv=False)
                add(form, "stream", L, p=0.5, extras=True, adv=False)
                add(form, "stream", L, causal=False, p=0.5 if n % 2 else 0.1, extras=True, adv=False)
    for L in (16, 17, 64):
        add("stream4", "auto", L, extras=True)
    for L in (65, 208):
        add("stream13", "auto", L, extras=True)
    # ---- streaming, every head size: every (ADV, HALF, PRE) at an on-edge, a one-past / tail and a past-the-tail length ------
    for dh in (16, 32, 64, 128):
        for form, lengths in (("stream4", (48, 49, 53)), ("stream13", (208, 65))):
            for adv in (True, False):
                for p in (0.5, 0.1):
                    for extras in (True, False):
                        for L in lengths:
                            add(form, "stream", L, dh=dh, causal=adv or p == 0.5, p=p, extras=extras, adv=adv)
    # ---- LDS-staged pair ---------------------------------------------------------------------------------------------------
    for form, lengths, edge in (("dma", DMA_L, (64, 49)), ("fast", FAST_L, (48, 33))):
        for n, L in enumerate(lengths):
            add(form, "staged", L)
            add(form, "staged", L, causal=False, p=0.1)
            add(form, "staged", L, causal=n % 2 == 0, p=0.0, adv=False)
        add(form, "staged", edge[0], extras=True)  # gate probabilities (the staged kernels read no affine planes)
        for dh in (16, 64):
            for L in edge:
                add(form, "staged", L, dh=dh)
                add(form, "staged", L, dh=dh, causal=False, p=0.1, adv=False)
    # ---- general kernel: counter RNG when pinned, explicit randomness on its own ----------------------------------------------
    for n, L in enumerate(GENERAL_L):
        add("general", "general", L)
        add("general", "auto", L, causal=False, p=0.1, kind="general")
        add("general", "general", L, causal=n % 2 == 0, p=0.0, adv=False)
    for dh in (16, 64, 128):
        for L in (64, 65):
            add("general", "general", L, dh=dh)
    add("general", "staged", 48, dh=128)  # the staged pair has no head size 128
    add("general", "staged", 49, dh=128)
    for L in (17, 65):
        opt = dict(kind="general")
        add("general", "auto", L, tag="fixed", combine="fixed", **opt)
        add("general", "auto", L, tag="annealing_037", combine="annealing", anneal_rate=0.37, **opt)
        add("general", "auto", L, tag="one_level_fixed", two_level=False, rich="fixed", **opt)
        add("general", "auto", L, tag="one_level_trainable", two_level=False, rich="trainable", **opt)
        add("general", "auto", L, tag="dense_LL", mask="dense_LL", **opt)
        add("general", "auto", L, tag="dense_L", mask="dense_L", causal=False, **opt)
        add("general", "auto", L, tag="order_only", terms=("order",), **opt)
        add("general", "auto", L, tag="distance_only", terms=("distance",), **opt)
    # ---- long form, pinned ---------------------------------------------------------------------------------------------------
    for n, L in enumerate(LONG_L):
        add("long", "long", L)
        add("long", "long", L, causal=False, p=0.1, extras=True)
        add("long", "long", L, causal=n % 2 == 0, p=0.0, adv=False)
    for dh in (16, 64, 128):
        for L in (64, 65):
            add("long", "long", L, dh=dh)
    return cases


CASES = _table()


def problem_key(c):
    """What the inputs and the oracle depend on: not the kernel that runs, nor whether the producer hands over extras."""
    return c._replace(id="", form="", fpin="", extras=False, kind="", adversarial=True)
