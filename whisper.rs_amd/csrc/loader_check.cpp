// loader_check.cpp — the host-only unit (wmi_host.cpp) as a program of its own,
// built with ASan + UBSan by `make loader_check`: no device, nothing preloaded.
//
//   loader_check PATH...
// Each *.wav path goes through read_wav, any other through parse_file; one
// line per path, "<path>\t<status>\t<message>".  Exit status 0 whatever the
// statuses (a sanitizer report aborts), 2 on a usage error.
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "wmi_host.h"

using namespace wmi;

static size_t file_size(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 0;
    fseek(f, 0, SEEK_END);
    const long end = ftell(f);
    fclose(f);
    return end > 0 ? (size_t)end : 0;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s PATH...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        const char *path = argv[i];
        const size_t n = strlen(path);
        std::string err;
        int rc;
        if (n >= 4 && !strcmp(path + n - 4, ".wav")) {
            size_t ns = 0;
            rc = read_wav(path, nullptr, 0, &ns, nullptr, nullptr, err);
            // the claimed count as capacity, a buffer no larger than the file: a data
            // chunk beyond the file must be refused before a sample is written
            std::vector<int16_t> pcm(std::min(ns, file_size(path) / 2 + 1));
            if (!rc) rc = read_wav(path, pcm.data(), ns, &ns, nullptr, nullptr, err);
        } else {
            ParsedModel pm;
            rc = parse_file(path, pm, err);
        }
        printf("%s\t%d\t%s\n", path, rc, err.c_str());
    }
    return 0;
}
