"""`targetdiff_amd.run.install`: the attribute swap that lets the reference's scripts run unmodified on the mirror class.

The reference checkout is a stand-in written here (``models/molopt_score_model.py`` with the two names the swap replaces), so the
test needs nothing outside the repository.  Running the reference's own ``scripts/sample_diffusion.py`` through
``python -m targetdiff_amd.run`` needs a real checkout: ``oracle/check_with_reference.py``."""
import sys

STAND_IN = '''class ScorePosNet3D:
    pass


def get_refine_net(refine_net_type, config):
    return None
'''


def test_install_is_idempotent_and_keeps_the_reference_class_reachable(tmp_path, monkeypatch):
    from targetdiff_amd import models, run
    (tmp_path / 'models').mkdir()
    (tmp_path / 'models' / '__init__.py').write_text('')
    (tmp_path / 'models' / 'molopt_score_model.py').write_text(STAND_IN)
    for name in [k for k in sys.modules if k == 'models' or k.startswith('models.')]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setattr(sys, 'path', list(sys.path))
    ref = run.install(str(tmp_path))
    assert ref.__file__ == str(tmp_path / 'models' / 'molopt_score_model.py')
    assert ref.ScorePosNet3D is models.ScorePosNet3D and ref.get_refine_net is models.get_refine_net
    kept = ref._reference_ScorePosNet3D
    assert kept is not None and kept is not models.ScorePosNet3D and kept.__module__ == 'models.molopt_score_model'
    assert run.install() is ref and ref._reference_ScorePosNet3D is kept
    run.uninstall()                   # leave the reference module as other tests expect it
    assert ref.ScorePosNet3D is kept and not hasattr(ref, '_reference_ScorePosNet3D')
