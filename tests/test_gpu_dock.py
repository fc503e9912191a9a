"""td_score_dock on the GPU (csrc/relax.hip) against td_score_minimize, td_score_report and tests/_dock_ref.py (held to its contract on the
host, tests/test_dock_host.py).  A rigid-body global search under this project's heuristic score, not AutoDock Vina's dock: three
translations and three rotations, no torsions.

The trajectory of a descent is not compared with the restatement's (the 6 x 6 algebra is not specified to the bit, tests/test_gpu_relax.py),
so a search is held to what follows from the contract whatever the trajectories: one chain without a round is td_score_minimize byte for
byte; the written terms are the score of the written coordinates; the coordinates are the transform's, bit for bit; the search is never
worse than the relaxation; the winner is the first argmin of the chains and the outputs are its; a chain does not depend on how many
chains run beside it, and its best does not rise with more rounds.  With max_steps = 0 a round is one evaluation of a mutated pose, and
there the chain states are the restatement's bit for bit wherever no decision is closer than the two evaluations can differ.

  1. the grids of test_gpu_score.py at 4 chains x 3 rounds;  2. the list against the walk, repeatability, the boundaries;  3. the
  restatement at max_steps = 0;  4. the redocking copies of the host test on 1h36;  5. quality.
"""
import types

import numpy as np
import pytest
import torch

import _dock_ref as DR
import _interactions_ref as IR
import _relax_ref as RR
import _score_ref as SR
from targetdiff_amd import capi, quality
from test_dock_host import REDOCK_SEED, redocking_copies
from test_gpu_relax import AROMATIC, CLASS_Z, N_P, PACKS, RSUM, W, _dev, check_terms, docked, evaluated, fixture_case, grid_case, rmsd, tensors
from test_gpu_relax import run as minimize, score

pytestmark = pytest.mark.gpu

C, R = 4, 3
IDENTITY = np.asarray([1.0, 0, 0, 0, 0, 0, 0])
CHAIN_KEYS = ('chain_terms', 'chain_transform', 'chain_accepts', 'chain_evals')


def uniforms(c, n_chains, n_rounds, seed):
    S, B = c['pos'].shape[0], len(c['ptr']) - 1
    return np.random.default_rng(seed).random((S, B, n_chains, n_rounds + 1, 7))


def dock(c, draws, check=False, **kw):
    """capi.score_dock of a case's numpy arrays with the draws [S, B, C, R + 1, 7], as numpy (no rotor inputs: n_rot is None)"""
    pack, pocket = tensors(c)
    d = torch.as_tensor(np.ascontiguousarray(draws), dtype=torch.float64, device=_dev())
    out = capi.score_dock(*pack, *pocket, W, check=check, n_chains=draws.shape[2], n_rounds=draws.shape[3] - 1, draws=d, **kw)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}


def energies(terms):
    return np.asarray([RR.energy(t, W) for t in terms.reshape(-1, 5)]).reshape(terms.shape[:-1])


@pytest.mark.parametrize('pack', list(PACKS))
@pytest.mark.parametrize('n_p', N_P)
def test_one_chain_without_a_round_is_score_minimize(n_p, pack):
    c, _, _ = grid_case(n_p, pack)
    m, d = minimize(c), dock(c, uniforms(c, 1, 0, 1))
    for k in RR.KEYS:
        if m[k] is not None:
            assert d[k].tobytes() == m[k].tobytes(), k
    assert d['n_rot'] is None and not d['best_chain'].any() and (d['chain_accepts'] == 1).all()
    np.testing.assert_array_equal(d['chain_terms'][:, :, 0], m['terms'])
    np.testing.assert_array_equal(d['chain_transform'][:, :, 0], m['transform'])
    np.testing.assert_array_equal(d['chain_evals'][:, :, 0], m['n_evals'])


@pytest.mark.parametrize('pack', list(PACKS))
@pytest.mark.parametrize('n_p', N_P)
def test_the_search_on_the_grid(n_p, pack):
    c, pr, mols = grid_case(n_p, pack)
    draws = uniforms(c, C, R, 1000 + n_p)
    m, d = minimize(c), dock(c, draws)
    tag = f'N_p = {n_p}, {pack}'
    # the input pose's integers are the relaxation's; the search is never worse than the relaxation, chain 0 begins with it
    np.testing.assert_array_equal(d['terms_in'], m['terms_in'])
    np.testing.assert_array_equal(d['grad_in'], m['grad_in'])
    e_chain, e = energies(d['chain_terms']), energies(d['terms'])
    assert (e <= energies(m['terms'])).all() and (e_chain[:, :, 0] <= energies(m['terms'])).all(), tag
    # the winner is the first argmin of the chains, and the outputs are that chain's
    np.testing.assert_array_equal(d['best_chain'], e_chain.argmin(-1))
    win = d['best_chain'][..., None, None].astype(np.int64)
    np.testing.assert_array_equal(d['terms'], np.take_along_axis(d['chain_terms'], win, 2)[:, :, 0])
    np.testing.assert_array_equal(d['transform'], np.take_along_axis(d['chain_transform'], win, 2)[:, :, 0])
    np.testing.assert_array_equal(d['n_evals'], d['chain_evals'].sum(-1))
    assert (d['chain_accepts'] >= 1).all() and (d['chain_accepts'] <= R + 1).all() and (d['chain_evals'] >= R + 1).all()
    assert (d['chain_evals'] <= (R + 1) * 257).all() and (d['n_steps'] <= d['n_evals']).all() and not (d['status'] & ~7).any()
    terms_at, pairs_at = score(c, d['pos'])
    same_roles = 0
    for (s, g), mol in mols.items():
        a, b, lel, lrole, scored = mol
        x, y, t = c['pos'][s, a:b], d['pos'][s, a:b], d['transform'][s, g]
        # the coordinates are the transform's, bit for bit; the identity keeps the input's bytes
        if (t == IDENTITY).all():
            assert y.tobytes() == x.tobytes(), (tag, s, g)
        else:
            np.testing.assert_array_equal(y, RR.transformed(x, scored, t), err_msg=f'{tag}, molecule {s, g}')
        assert abs(float((d['chain_transform'][s, g, :, :4] ** 2).sum(-1).max()) - 1.0) < 1e-12
        assert (np.sqrt((d['chain_transform'][s, g, :, 4:] ** 2).sum(-1)) <= 3.0).all(), (tag, s, g)
        # the written terms are the score of the written coordinates under the input pose's roles (tests/test_gpu_relax.py) ...
        w_terms, _, w_pairs = evaluated(c, pr, mol, y)
        assert w_pairs == d['n_pairs'][s, g], (tag, s, g)
        check_terms(d['terms'][s, g], w_terms, w_pairs, f'{tag}, molecule {s, g}')
        # ... and td_score_report's own integers there, wherever typing the written pose anew gives the input pose's roles
        if np.array_equal(RR.molecule_inputs(y, c['v'][s, a:b], CLASS_Z)[1], lrole):
            same_roles += 1
            np.testing.assert_array_equal(d['terms'][s, g], terms_at[s, g], err_msg=f'{tag}, molecule {s, g}')
            assert d['n_pairs'][s, g] == pairs_at[s, g]
    assert same_roles > len(mols) // 2, 'td_score_report is compared for most molecules'
    # a chain does not depend on the chains beside it ...
    two = dock(c, draws[:, :, :2])
    for k in CHAIN_KEYS:
        assert two[k].tobytes() == np.ascontiguousarray(d[k][:, :, :2]).tobytes(), k
    # ... and its best does not rise with more rounds on a prefix of the draws
    short = dock(c, draws[:, :, :, :2])
    assert (e_chain <= energies(short['chain_terms'])).all(), tag
    if n_p >= 64:
        assert (d['best_chain'] > 0).any() or (e_chain[:, :, 0] < energies(m['terms'])).any(), 'no case passes vacuously'
        assert (d['chain_accepts'] > 1).any() and (d['transform'] != IDENTITY).any()
    print(f'{tag}: best chains {d["best_chain"].tolist()}, evaluations {d["n_evals"].tolist()}, gain over the relaxation '
          f'{(energies(m["terms"]) - e).max():.4f} at most')


def test_the_walk_in_global_memory_and_a_second_run_give_identical_bytes():
    c = IR.build_case(11, 300, [5, 70, 0, 31, 129], S=2)
    draws = uniforms(c, C, R, 3)
    listed, again = dock(c, draws), dock(c, draws)
    assert (listed['n_steps'] > 0).any() and (listed['best_chain'] > 0).any()
    for capacity, other in ((None, again), (0, dock(c, draws, _list_capacity=0)), (64, dock(c, draws, _list_capacity=64))):
        for k in DR.KEYS:
            if listed[k] is not None:
                assert other[k].tobytes() == listed[k].tobytes(), (capacity, k)


def test_an_oversize_molecule_empty_packs_an_empty_pocket_and_no_scored_atom():
    c = IR.build_case(5, 130, [20, 513, 33], S=2)
    draws = uniforms(c, C, R, 4)
    with pytest.raises(ValueError, match='at most 512'):
        dock(c, draws, check=True)
    r = dock(c, draws, max_steps=8)
    assert (r['n_pairs'][:, 1] == -1).all() and (r['status'][:, 1] == -1).all() and not r['n_steps'][:, 1].any() and not r['n_evals'][:, 1].any()
    assert (r['terms'][:, 1] == SR.INT64_MIN).all() and (r['terms_in'][:, 1] == SR.INT64_MIN).all() and not r['grad_in'][:, 1].any()
    assert (r['chain_terms'][:, 1] == SR.INT64_MIN).all() and (r['chain_transform'][:, 1] == IDENTITY).all() and not r['best_chain'][:, 1].any()
    assert not r['chain_accepts'][:, 1].any() and not r['chain_evals'][:, 1].any() and (r['transform'][:, 1] == IDENTITY).all()
    assert r['pos'][:, 20:533].tobytes() == c['pos'][:, 20:533].tobytes()
    alone = dict(c, pos=np.concatenate([c['pos'][:, :20], c['pos'][:, 533:]], 1), v=np.concatenate([c['v'][:, :20], c['v'][:, 533:]], 1),
                 ptr=np.asarray([0, 20, 53], np.int32))
    a = dock(alone, draws[:, [0, 2]], max_steps=8)
    assert (a['n_steps'] > 0).any()
    for k in DR.KEYS[3:]:
        np.testing.assert_array_equal(a[k], r[k][:, [0, 2]], err_msg=k)
    np.testing.assert_array_equal(a['pos'], np.concatenate([r['pos'][:, :20], r['pos'][:, 533:]], 1))
    for S, sizes in ((0, [4, 9]), (2, [])):
        e = IR.build_case(1, 70, sizes, S=S)
        r = dock(e, uniforms(e, C, R, 5))
        assert r['terms'].shape == (S, len(sizes), 5) and r['chain_transform'].shape == (S, len(sizes), C, 7) and r['pos'].tobytes() == e['pos'].tobytes()
    e = IR.build_case(1, 0, [4, 9], S=2)                                         # N_p = 0: every energy is zero, the input pose wins
    r = dock(e, uniforms(e, C, R, 6))
    assert not r['terms'].any() and not r['n_pairs'].any() and not r['n_steps'].any() and (r['n_evals'] == C * (R + 1)).all()
    assert not r['best_chain'].any() and (r['transform'] == IDENTITY).all() and r['pos'].tobytes() == e['pos'].tobytes()
    c = IR.build_case(11, 300, [5, 70, 0, 31, 129], S=2)
    c['v'][:, :5] = 0                                                            # a molecule of hydrogens: no scored atom
    r = dock(c, uniforms(c, C, R, 7))
    assert not r['n_steps'][:, 0].any() and r['pos'][:, :5].tobytes() == c['pos'][:, :5].tobytes() and not r['best_chain'][:, [0, 2]].any()
    pack, pocket = tensors(c)
    for kw, match in ((dict(n_chains=0), 'n_chains'), (dict(n_chains=65), 'n_chains'), (dict(n_rounds=-1), 'n_rounds'), (dict(n_rounds=257), 'n_rounds'),
                      (dict(amplitude=0.0), 'amplitude'), (dict(temperature=float('nan')), 'temperature'), (dict(max_shift=0.0), 'max_shift'),
                      (dict(draws=torch.zeros(3, dtype=torch.float64, device=_dev())), 'draws')):
        with pytest.raises(ValueError, match=match):
            capi.score_dock(*pack, *pocket, W, **kw)
    seeded = [capi.score_dock(*pack, *pocket, W, n_chains=2, n_rounds=1, seed=s, check=False) for s in (5, 5, 6)]
    assert torch.equal(seeded[0]['draws'], seeded[1]['draws']) and not torch.equal(seeded[0]['draws'], seeded[2]['draws'])
    assert torch.equal(seeded[0]['chain_terms'], seeded[1]['chain_terms']) and seeded[0]['draws'].shape == (2, 5, 2, 2, 7)


def test_with_zero_steps_the_chain_states_are_the_restatements_bit_for_bit():
    """max_steps = 0: a round is one evaluation of a mutated pose, so a chain is its mutations and its decisions.  An evaluation's
    integers differ from the restatement's by at most one unit of 2^-24 per counted pair in the two Gaussian terms (only exp differs),
    so inter by at most (|w0| + |w1|) units per pair, and a decision compares two such energies.  A molecule of n atoms counts at most
    n N_p pairs.  Chains none of whose decisions is closer than that are compared: the transform bit for bit, terms 2-4 exactly, terms
    0-1 within a unit per counted pair."""
    n_p = 300
    c = IR.build_case(11, n_p, [5, 70, 0, 31, 129], S=2)
    draws = uniforms(c, C, R, 8)
    d = dock(c, draws, max_steps=0)
    w = DR.score_dock(c['pos'], c['v'], c['ptr'], CLASS_Z, AROMATIC, c['ppos'], c['pelem'], c['pkind'], c['prole'], 40, RSUM, W, with_rotors=False,
                      max_steps=0, n_chains=C, n_rounds=R, draws=draws)
    np.testing.assert_array_equal(d['chain_evals'], w['chain_evals'])
    assert (d['chain_evals'] == R + 1).all() and not d['n_steps'].any()
    compared = selected = 0
    for s in range(2):
        for g in range(5):
            a, b = int(c['ptr'][g]), int(c['ptr'][g + 1])
            bound = 2.0 * (b - a) * n_p * (abs(W[0]) + abs(W[1])) / SR.UNIT
            clear = w['margin'][s, g] > bound
            for k in np.nonzero(clear)[0]:
                tag = f'molecule {s, g}, chain {k}'
                np.testing.assert_array_equal(d['chain_transform'][s, g, k], w['chain_transform'][s, g, k], err_msg=tag)
                assert d['chain_accepts'][s, g, k] == w['chain_accepts'][s, g, k], tag
                check_terms(d['chain_terms'][s, g, k], w['chain_terms'][s, g, k], int(w['chain_pairs'][s, g, k]), tag)
                compared += 1
            e = np.sort(energies(w['chain_terms'][s, g]))
            if clear.all() and e[1] - e[0] > bound:
                selected += 1
                assert d['best_chain'][s, g] == w['best_chain'][s, g] and d['n_pairs'][s, g] == w['n_pairs'][s, g]
                np.testing.assert_array_equal(d['transform'][s, g], w['transform'][s, g])
                np.testing.assert_array_equal(d['pos'][s, a:b], w['pos'][s, a:b])
                assert d['status'][s, g] == w['status'][s, g]
    print(f'{compared} of {2 * 5 * C} chains compared, the selection of {selected} of 10 molecules')
    assert compared >= 2 * 5 * C // 2 and selected >= 3, 'the draws leave most chains clear of a close decision'


def test_redocking_on_1h36_finds_the_planted_pose_that_the_relaxation_alone_misses():
    """The copies, the draws and the bounds of tests/test_dock_host.py: the relaxation alone ends more than 2 A RMSD from x*, the search
    at 16 x 16 within 0.25 A."""
    _, lpos, lv = docked()
    n = len(lv)
    star = minimize(fixture_case([lpos], lv), max_steps=200)
    x_star, e_star = star['pos'][0], RR.energy(star['terms'][0, 0], W)
    copies = redocking_copies(x_star, lv)
    c = fixture_case(copies, lv)
    draws = np.stack([np.random.default_rng(REDOCK_SEED).random((16, 17, 7)) for _ in copies])[None]
    local, d = minimize(c), dock(c, draws)
    for g in range(len(copies)):
        alone, found = rmsd(local['pos'][0, g * n:(g + 1) * n], x_star), rmsd(d['pos'][0, g * n:(g + 1) * n], x_star)
        e = energies(d['chain_terms'][0, g])
        print(f'copy {g}: start {rmsd(copies[g], x_star):.3f} A; the relaxation alone ends {alone:.3f} A from x* at '
              f'{RR.energy(local["terms"][0, g], W):.4f}; the search {found:.4f} A at {e.min():.4f} (E* {e_star:.4f}), chain '
              f'{d["best_chain"][0, g]}, {int((e < e.min() + 0.5).sum())} of 16 chains agree, {d["n_evals"][0, g]} evaluations')
        assert alone > 2.0, g
        assert found <= 0.25, g


EXACT = ('n_included', 'scored', 'sum_evals', 'n_samples', 'n_ref')


def test_pocket_dock_the_pack_and_sample_dock_through_a_result_dictionary():
    dev = _dev()
    p, lpos, lv = docked()
    rng = np.random.default_rng(0)
    # three samples: the docked pose, a jittered copy, and a part of it moved 30 A away; two frames that end in those poses
    final = [lpos, (lpos + rng.normal(0, 0.5, lpos.shape)).astype(np.float32), lpos[:17] + np.float32(30)]
    pos_traj = [np.stack([(x + rng.normal(0, 0.3 * (1 - t), x.shape)).astype(np.float32) for t in range(2)]).astype(np.float64) for x in final]
    v_traj = [np.stack([lv[:len(x)]] * 2) for x in final]
    data = types.SimpleNamespace(protein_pos=torch.from_numpy(p['pos']), protein_atom_feature=torch.from_numpy(p['feat'].astype(np.int64)))
    result = {'data': data, 'pred_ligand_pos_traj': pos_traj, 'pred_ligand_v_traj': v_traj}
    elem, kind, _ = quality.pocket_kinds(p['feat'])
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    pocket = (t(p['pos'], torch.float32), t(elem, torch.int32), t(kind, torch.int32), t(IR.pocket_roles(p['feat']), torch.int32), 40, RSUM, W)
    search = dict(n_chains=C, n_rounds=R, seed=9)

    def raw_outputs(pos, v, ptr):
        pack = (t(pos, torch.float32), t(v, torch.int64), t(ptr, torch.int32), CLASS_Z, AROMATIC)
        bond_ptr = capi.bond_graph(*pack, (), None, False, True)['bond_ptr']
        ring = capi.ring_report(*pack, None, bond_ptr, False)['bond_ring']
        out = capi.score_dock(*pack, *pocket, 8.0, 1.75, bond_ptr, ring, **search)
        low = capi.score_minimize(*pack, *pocket, 8.0, 1.75, bond_ptr, ring)
        return {k: x.cpu().numpy() for k, x in out.items()}, {k: x.cpu().numpy() for k, x in low.items()}

    q, _ = raw_outputs(lpos[None], lv[None], [0, len(lv)])
    ref_score = float(SR.energies(q['terms'], q['n_rot'])[2][0, 0])
    pos = np.concatenate([x[1:] for x in pos_traj], 1).astype(np.float32)
    v = np.concatenate([x[1:] for x in v_traj], 1)
    raw, raw_min = raw_outputs(pos, v, [0, 25, 50, 67])
    expect = quality.DockReport.from_outputs(raw, raw_min, np.ones((1, 3), bool), pos, [25, 25, 17], ref_score=ref_score)
    got = quality.sample_dock(result, reference_ligand=(lpos, lv), device=dev, **search)
    pack = quality.SamplePack(result, -1, device=dev)
    method = pack.dock(data, reference_ligand=(lpos, lv), **search)
    assert pack.docked_pos.cpu().numpy().tobytes() == raw['pos'].tobytes()
    for rep in (got, method):
        assert vars(rep).keys() == vars(expect).keys()
        for k, x in vars(expect).items():
            if k in EXACT:
                np.testing.assert_array_equal(getattr(rep, k), x, err_msg=k)
            else:
                np.testing.assert_allclose(getattr(rep, k), x, rtol=1e-6, atol=0, err_msg=k)
        a, b = rep.summary(-1), expect.summary(-1)
        assert a.keys() == b.keys()
        for k in b:
            np.testing.assert_allclose(a[k], b[k], rtol=1e-6, atol=0, err_msg=k)
    s = got.summary(-1)
    assert s['mean_score_dock'] <= s['mean_score_min'] < s['mean_score'] and s['mean_gain_dock'] >= 0 and s['better_than_ref_dock'] <= 1 / 3
    assert s['best_score_dock'] <= s['median_score_dock'] and 0 < s['mean_rmsd_dock'] and 0 < s['chains_agree'] <= 1 and s['mean_evals_dock'] > C * (R + 1)
    np.testing.assert_allclose(s['ref_score_dock'], ref_score, rtol=1e-6)
    with pytest.raises(ValueError, match='long-lived workgroups'):
        quality.sample_dock(result, 'all', device=dev)
    # the stateless form gives the kernel's outputs on the same pocket
    x = quality.pocket_dock(p['pos'], p['feat'], pos[0], v[0], ligand_ptr=torch.tensor([0, 25, 50, 67], dtype=torch.int32), device=dev, **search)
    for k, a in (('raw_terms_in', raw['terms_in']), ('raw_terms', raw['terms']), ('n_pairs', raw['n_pairs']), ('n_rot', raw['n_rot']),
                 ('n_evals', raw['n_evals']), ('status', raw['status']), ('transform', raw['transform']), ('best_chain', raw['best_chain']),
                 ('chain_terms', raw['chain_terms']), ('chain_accepts', raw['chain_accepts'])):
        np.testing.assert_array_equal(getattr(x, k), a, err_msg=k)
    assert x.pos.cpu().numpy().tobytes() == raw['pos'].tobytes()
    np.testing.assert_allclose(x.score, SR.energies(raw['terms'], raw['n_rot'])[2], rtol=1e-6)
    np.testing.assert_allclose(x.score_min, SR.energies(raw_min['terms'], raw_min['n_rot'])[2], rtol=1e-6)
    assert x.rmsd[0, 2] == 0 and x.rmsd[0, 0] > 0 and (x.score <= x.score_min).all()
