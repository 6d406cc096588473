// png16_test.cpp -- include/xfeat/image_io.h load_png16 on a file: the samples to stdout in host byte order (exit 0), exit 1 when the
// reader refuses the file, exit 3 when the 8-bit loader accepts it (it must keep refusing 16-bit files).  Built with ASan + UBSan.
#include <cstdio>
#include "xfeat/image_io.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    xfeat::Image16 im;
    xfeat::Image8 i8;
    const bool as8 = xfeat::load_png(argv[1], i8);
    if (!xfeat::load_png16(argv[1], im)) return 1;
    if (as8) return 3;
    fwrite(im.data.data(), 2, im.data.size(), stdout);
    return 0;
}
