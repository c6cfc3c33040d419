// Host build of the JPEG encode arithmetic in svgrasterize.py_amd/csrc/svgr_core.h (jpeg_group, jpeg_fdct_block, jpeg_coefficient
// through jpeg_encode_frame), for CPU-side unit tests only (tests/test_jpeg_encode_host.py, tests/test_gpu_jpeg_encode.py).
// NOT a CPU fallback of the product: the package never loads it.
#include <vector>

#include "../include/svgr.h"
#include "../svgrasterize.py_amd/csrc/svgr_core.h"

using namespace svgr;

extern "C" {

// what svgr_jpeg_encode computes: rgba[height * width * 4], quant[n_comp][64], coef in the layout of include/svgr.h.  If
// `samples` is not null it receives the MCU-padded planes, component after component (64 bytes per block).  Returns 0, or -1
// for a frame svgr_jpeg_encode does not take.
int jeh_encode(const svgr_jpeg_frame* f, const uint8_t* rgba, const uint16_t* quant, uint8_t* samples, int16_t* coef) {
    if ((f->n_comp != 1 && f->n_comp != 3) || f->width < 1 || f->height < 1) return -1;
    if (f->h[0] < 1 || f->h[0] > 2 || f->v[0] < 1 || f->v[0] > 2) return -1;
    if (f->n_comp == 1 && (f->h[0] != 1 || f->v[0] != 1)) return -1;
    if (f->n_comp == 3 && (f->h[1] != 1 || f->v[1] != 1 || f->h[2] != 1 || f->v[2] != 1)) return -1;
    const int H = f->h[0], V = f->v[0];
    const int64_t mcus = (int64_t)((f->width + 8 * H - 1) / (8 * H)) * ((f->height + 8 * V - 1) / (8 * V));
    std::vector<uint8_t> own;
    if (!samples) {
        own.resize((size_t)mcus * 64 * (H * V + 2));
        samples = own.data();
    }
    jpeg_encode_frame(reinterpret_cast<const uint32_t*>(rgba), f->width, f->height, f->n_comp, H, V, quant, samples, coef);
    return 0;
}

}  // extern "C"
