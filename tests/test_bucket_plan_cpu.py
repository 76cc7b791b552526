"""resident.plan_batches / shard_batches / padded_ratio: host arithmetic on the size table, no GPU.  The ratio conditions use the size
draw of tools/ragged_train_throughput.py (heights 128-256, widths 568-4064) for N = 25 691 samples, the size of GrandStaff's train
split, in batches of 32.  A numpy restatement of the three arrangements gave real / padded = 0.445 (random batches), 0.742 (chunks
of 32 batches sorted by width) and 0.977 (one height, sorted chunks); the bounds below leave room for another generator's draw."""
import functools

import torch

from omr_a2s_multimodal_transformer_amd.resident import padded_ratio, plan_batches, shard_batches

N_BIG, BATCH = 25691, 32
BUDGET = 32 * 256 * 2048


def draw(n, seed, one_height=False):
    g = torch.Generator().manual_seed(seed)
    h = torch.randint(128, 257, (n,), generator=g)
    w = torch.randint(568, 4065, (n,), generator=g)
    if one_height:
        h = torch.full_like(h, 128)
    return torch.stack([h, w], dim=1)


@functools.lru_cache(maxsize=None)
def big():
    return draw(N_BIG, 2024)


@functools.lru_cache(maxsize=None)
def big_plan(chunk_batches, budget=None):
    return plan_batches(big(), BATCH, chunk_batches=chunk_batches, max_padded_pixels=budget, seed=5)


def plane_pixels(batch, sizes):
    s = sizes[batch]
    return len(batch) * int(s[:, 0].max()) * int(s[:, 1].max())


def test_every_sample_appears_exactly_once():
    sizes = draw(1000, 1)
    for kw in (dict(), dict(chunk_batches=1), dict(max_padded_pixels=8 * 200 * 2000), dict(chunk_batches=3, max_padded_tokens=100, target_lens=list(range(1, 1001)))):
        plan = plan_batches(sizes, 16, seed=3, **kw)
        assert sorted(n for b in plan for n in b) == list(range(1000)), kw
        assert all(1 <= len(b) <= 16 for b in plan), kw
    assert sorted(n for b in big_plan(32) for n in b) == list(range(N_BIG))


def test_no_batch_exceeds_the_size_or_either_budget_unless_it_is_a_batch_of_one():
    sizes, sizes2 = draw(600, 2), draw(600, 3)
    g = torch.Generator().manual_seed(4)
    tl = torch.randint(5, 400, (600,), generator=g).tolist()
    px, tok = 6 * (256 * 3000 + 256 * 3000), 1500
    plan = plan_batches(sizes, 12, sizes2=sizes2, target_lens=tl, max_padded_pixels=px, max_padded_tokens=tok, chunk_batches=8, seed=9)
    assert sorted(n for b in plan for n in b) == list(range(600))
    for b in plan:
        assert len(b) <= 12
        if len(b) > 1:
            assert plane_pixels(b, sizes) + plane_pixels(b, sizes2) <= px, b
            assert len(b) * max(tl[n] for n in b) <= tok, b
    assert len({len(b) for b in plan}) > 1
    # each budget binds on its own: without the other one some batch breaks it
    assert any(plane_pixels(b, sizes) + plane_pixels(b, sizes2) > px
               for b in plan_batches(sizes, 12, sizes2=sizes2, target_lens=tl, max_padded_tokens=tok, chunk_batches=8, seed=9))
    assert any(len(b) * max(tl[n] for n in b) > tok for b in plan_batches(sizes, 12, sizes2=sizes2, max_padded_pixels=px, chunk_batches=8, seed=9))


def test_the_same_seed_and_epoch_give_the_same_plan_and_another_epoch_another():
    sizes = draw(500, 6)
    a = plan_batches(sizes, 8, seed=1, epoch=2)
    assert a == plan_batches(sizes.tolist(), 8, seed=1, epoch=2)
    assert a == plan_batches(sizes, 8, seed=3, epoch=0)                   # the generator is seeded with seed + epoch, as ddp.shard_indices does
    b = plan_batches(sizes, 8, seed=1, epoch=3)
    assert a != b and sorted(map(sorted, a)) != sorted(map(sorted, b))


def test_chunk_batches_1_reproduces_the_slices_of_the_permutation():
    sizes = draw(203, 7)
    plan = plan_batches(sizes, 10, chunk_batches=1, seed=4, epoch=1)
    perm = torch.randperm(203, generator=torch.Generator().manual_seed(5)).tolist()
    slices = [sorted(perm[i:i + 10]) for i in range(0, 203, 10)]
    assert sorted(sorted(b) for b in plan) == sorted(slices)
    assert [sorted(b) for b in plan] != slices                            # step 5: the batches' order is shuffled
    for b in plan:                                                        # step 3: inside a batch, by (width, height)
        keys = [(int(sizes[n, 1]), int(sizes[n, 0])) for n in b]
        assert keys == sorted(keys)


def test_shard_batches_gives_every_rank_the_same_count_and_covers_the_plan():
    plan = plan_batches(draw(333, 8), 4, max_padded_pixels=4 * 200 * 2500, seed=2)
    for world in (2, 3):
        shards = [shard_batches(plan, r, world) for r in range(world)]
        steps = (len(plan) + world - 1) // world
        assert [len(s) for s in shards] == [steps] * world
        interleaved = [shards[i % world][i // world] for i in range(steps * world)]
        assert interleaved[:len(plan)] == plan
        assert interleaved[len(plan):] == plan[:steps * world - len(plan)]            # wrap-around padding
    assert shard_batches(plan, 0, 1) == plan
    seven = [[i] for i in range(7)]                                       # 7 batches: world 2 pads one, world 3 pads two
    assert shard_batches(seven, 1, 2) == [[1], [3], [5], [0]]
    assert [shard_batches(seven, r, 3) for r in range(3)] == [[[0], [3], [6]], [[1], [4], [0]], [[2], [5], [1]]]


def test_an_oversize_sample_is_kept_alone_in_its_batch():
    sizes = torch.tensor([[100, 600], [256, 4064], [100, 610], [100, 620], [100, 630]])
    plan = plan_batches(sizes, 4, max_padded_pixels=4 * 100 * 640, seed=0)
    assert sorted(n for b in plan for n in b) == [0, 1, 2, 3, 4]
    assert [1] in plan and sorted(map(sorted, plan)) == [[0, 2, 3, 4], [1]]
    tl = [5, 6, 500, 7, 8]
    plan = plan_batches(sizes, 4, target_lens=tl, max_padded_tokens=40, seed=0)
    assert [2] in plan and sorted(n for b in plan for n in b) == [0, 1, 2, 3, 4]


def test_random_batches_waste_more_than_half_of_the_plane():
    r = padded_ratio(big_plan(1), big())
    print(f"real / padded, random batches of {BATCH}: {r:.3f}")
    assert r <= 0.50


def test_sorted_chunks_of_32_batches_keep_70_percent_real():
    r = padded_ratio(big_plan(32), big())
    print(f"real / padded, chunks of 32 batches sorted by width: {r:.3f}")
    assert r >= 0.70


def test_one_height_and_sorted_chunks_keep_95_percent_real():
    sizes = draw(N_BIG, 2024, one_height=True)
    r = padded_ratio(plan_batches(sizes, BATCH, chunk_batches=32, seed=5), sizes)
    print(f"real / padded, all heights 128, chunks of 32 batches sorted by width: {r:.3f}")
    assert r >= 0.95


def test_a_pixel_budget_holds_for_every_batch_and_varies_the_batch_size():
    """Budget 32 * 256 * 2048 pixels over chunks of 1 024 samples, batch_size 256 so that only the budget cuts (a restatement gave
    batches of 1-84 samples, mean 27)."""
    sizes = big()
    plan = plan_batches(sizes, 256, max_padded_pixels=BUDGET, chunk_batches=4, seed=5)
    assert sorted(n for b in plan for n in b) == list(range(N_BIG))
    lens = [len(b) for b in plan]
    over = [b for b in plan if len(b) > 1 and plane_pixels(b, sizes) > BUDGET]
    print(f"pixel budget {BUDGET}: {len(plan)} batches of {min(lens)}-{max(lens)} samples, mean {sum(lens) / len(lens):.1f}; "
          f"real / padded {padded_ratio(plan, sizes):.3f}")
    assert not over
    assert len(set(lens)) > 5 and max(lens) > 32 > min(lens)
    capped = big_plan(32, BUDGET)                                         # the same budget under batch_size 32
    assert all(len(b) <= BATCH and (len(b) == 1 or plane_pixels(b, sizes) <= BUDGET) for b in capped)
    assert len({len(b) for b in capped}) > 1
