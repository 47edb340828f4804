"""-m gpu: MPO files (a JPEG, an APP2 MPF index in it, more JPEGs behind its EOI; the mpo entry of the reference's IMG_FORMATS) through the JPEG
decoder.  No new decoder: jpeg.decode reads the first frame, which is what cv2.imread and Pillow open.  The fixtures (tests/golden/
bmp_cases.npz, written by Pillow with a second frame of another size) hold Pillow's decode of the first frame, stored BGR.  Bit-exact:
torch.equal.  No Pillow here.
"""
import pytest
import torch

import maf_yolo_amd as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def mpo(golden):
    z = golden("bmp_cases")
    names = [str(n) for n in z["mpo_names"]]
    return names, [z["mpofile_" + n].tobytes() for n in names], [torch.from_numpy(z["mpobgr_" + n]) for n in names]


def test_jpeg_decode_returns_the_first_frame(mpo):
    names, files, want = mpo
    assert len(names) >= 3
    got = M.jpeg.decode(files, device=DEV)
    for n, f, g, w in zip(names, files, got, want):
        assert M.frames.kind(f) == "jpeg" and tuple(g.shape) == tuple(w.shape), n
        assert torch.equal(g.cpu(), w), n
        assert torch.equal(M.jpeg.decode([f], device=DEV)[0], g), n


def test_the_router_takes_mpo_files_as_jpeg(mpo, golden):
    names, files, want = mpo
    png = golden("png_cases")
    pfile = png["file_" + str(png["names"][0])].tobytes()
    got = M.frames.decode([files[0], pfile] + files[1:], device=DEV)
    for n, g, w in zip(names, [got[0]] + got[2:], want):
        assert torch.equal(g.cpu(), w), n
    assert torch.equal(got[1], M.png.decode([pfile], device=DEV)[0])
    got, status = M.frames.decode(files, device=DEV, check=False, bmp=True)
    assert status.tolist() == [0] * len(files) and all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
