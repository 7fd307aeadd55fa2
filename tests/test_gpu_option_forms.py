"""Every entry point under each non-default build and order switch, and a switch between a build and an incremental call
(tests/option_forms.py has the forms, the scenarios and the shapes; tests/test_option_forms_cpu.py proves what they reach)."""
import pytest

from tests import option_forms as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scenario,form", F.PAIRS, ids=[f"{s}-{f}" for s, f in F.PAIRS])
def test_entry_point_under_a_form(scenario, form):
    F.SCENARIOS[scenario](F.FORMS[form], (), f"{scenario} under {form}")


@pytest.mark.parametrize("scenario,form,direction", F.LATE_CASES, ids=[f"{s}-{d}-{f}" for s, f, d in F.LATE_CASES])
def test_form_switched_on_a_built_context(scenario, form, direction):
    """"to": built and scored under the defaults, the form set, the call made; "from": the other way round.  The results are those
    of a context that had the final options from the start, and stay so when read and scored again."""
    options, late = F.late_options(form, direction)
    F.SCENARIOS[scenario](options, late, f"{scenario}, switched {direction} {form} on the built context")


def test_an_unknown_option_is_refused_and_changes_nothing():
    from pandelos_amd import _lib
    nat = F._mid_context((), ())
    ref = F.reference("mid")
    nat.score_all()
    before = nat.timings()
    launches = before["join_launches"]
    assert launches > 0
    for name in ("lean_radixx", "onepass-scan", "Lean_records", ""):
        with pytest.raises(_lib.PdlError) as e:
            nat.set_option(name, 0)
        assert e.value.code == _lib.PDL_ERR_ARGUMENT, name
    F.H.assert_scores_equal(nat.generate_scores_part(ref.genomes - 1).as_dict(), ref.scores(ref.genomes - 1), "after the refusals")
    assert nat.timings()["join_launches"] == launches and nat.timings() == before, "a refused option dropped the scores: a second pass ran"
    nat.close()
