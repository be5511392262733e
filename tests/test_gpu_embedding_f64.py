"""embedding_kernel and embedding_img_kernel of csrc/misc.hip on the GPU through eg_embedding, bit for bit (tests/misc_f64.py section 5): clamped
indices (-1, 0, n_words - 1, n_words, 2^40), a table whose unread rows are NaN, the pad columns (canary without images, +0 with them), the bf16 images
against eg_split_tiles of the same rows, the image slots of the last tile's rows past `rows` (canary) and the zero line."""
import pytest
import torch

import misc_f64 as M
import misc_gpu as G
import train_tail_gpu as D
from small_ops_f64 import image_rows, images_of

pytestmark = pytest.mark.gpu
_ID = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("case", M.EMB_CASES, ids=_ID)
def test_embedding_rows_are_the_table_rows_bit_for_bit(case):
    L, lib, ptr, st = D.api()
    rows, dim, ld = case
    idx, table = M.emb_inputs(case)
    want = M.emb_rows(idx, table)
    idx_d, table_d = idx.to(D.dev()), G.up_nan(table)
    what = f"embedding {case}"
    # without images: the columns dim .. ld-1 keep their canary
    out = D.Guarded((rows, ld))
    L.check(lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out.t), None, None, rows, dim, ld, M.EMB_WORDS, st), what)
    got = out.intact(what)
    assert torch.equal(G.bits(got[:, :dim]), G.bits(want)), what + ": rows differ from table[clamp(idx)]"
    assert bool((G.bits(got[:, dim:]) == D.SENTINEL).all()), what + ": pad columns written without images"
    # with images and the zero line
    mt = (rows + 63) // 64
    out, img, zero = D.Guarded((rows, ld)), D.Guarded((mt * 64 * ld,)), D.Guarded((32 * ld,))
    before = img.t.cpu().clone()
    L.check(lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out.t), ptr(img.t), ptr(zero.t), rows, dim, ld, M.EMB_WORDS, st), what + " images")
    got = out.intact(what + " images")
    assert torch.equal(G.bits(got[:, :dim]), G.bits(want)), what + ": rows differ from table[clamp(idx)] (images)"
    assert bool((G.bits(got[:, dim:]) == 0).all()), what + ": pad columns are not +0 with images"
    assert bool((G.bits(zero.intact(what + " zero line")) == 0).all()), what + ": the zero line is not cleared"
    as_tiles = lambda t: t.view(torch.int16).view(2, mt, ld // 8, 64, 8)
    tiles = as_tiles(img.intact(what + " images"))
    assert torch.equal(image_rows(tiles, rows), image_rows(images_of(got), rows)), what + ": images differ from the bf16 split of the rows"
    split = D.Guarded((mt * 64 * ld,))
    L.check(lib.eg_split_tiles(ptr(out.t), ld, rows, ld, ptr(split.t), st), what + " eg_split_tiles")
    assert torch.equal(image_rows(tiles, rows), image_rows(as_tiles(split.intact(what + " eg_split_tiles")), rows)), what + ": images differ from eg_split_tiles"
    assert torch.equal(image_rows(tiles, mt * 64)[:, rows:], image_rows(as_tiles(before), mt * 64)[:, rows:]), what + ": image slots past the last row were written"
    # the zero line is optional
    out2, img2 = D.Guarded((rows, ld)), D.Guarded((mt * 64 * ld,))
    L.check(lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out2.t), ptr(img2.t), None, rows, dim, ld, M.EMB_WORDS, st), what + " no zero line")
    assert torch.equal(G.bits(img2.intact(what)), G.bits(img.t.cpu())), what + ": the zero line changes the images"
    assert torch.equal(G.bits(out2.intact(what)), G.bits(got))


def test_embedding_refusals_write_nothing():
    L, lib, ptr, st = D.api()
    idx, table = M.emb_inputs((4, 8, 64))
    idx_d, table_d = idx.to(D.dev()), G.up_nan(table)
    out, img, zero = D.Guarded((4, 64)), D.Guarded((64 * 64,)), D.Guarded((32 * 64,))
    assert lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out.t), None, None, 4, 6, 64, M.EMB_WORDS, st) == -5          # dim % 4
    assert lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out.t), None, None, 4, 8, 4, M.EMB_WORDS, st) == -5           # ld < dim
    assert lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out.t), ptr(img.t), ptr(zero.t), 4, 8, 32, M.EMB_WORDS, st) == -5    # images with ld % 64
    assert lib.eg_embedding(ptr(idx_d), ptr(table_d), ptr(out.t), None, ptr(zero.t), 4, 8, 64, M.EMB_WORDS, st) == D.BAD_ARG  # zero line without images
    for o in (out, img, zero):
        o.untouched("refused eg_embedding")
