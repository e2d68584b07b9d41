// flow_hash_main <words> <file>: the flow table's hash (csrc/rss_flow_hash.h, compiled for the
// host) of every tuple of <words> little-endian uint32 in <file>, one hex word per line.
// tests/test_flow_aggregate.py compares tests/flow_hash.py with it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rss_flow_hash.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <3|9> <file>\n", argv[0]);
        return 2;
    }
    const int words = atoi(argv[1]);
    if (words != 3 && words != 9) {
        fprintf(stderr, "words must be 3 or 9\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) {
        perror(argv[2]);
        return 1;
    }
    std::vector<uint32_t> row(words);
    size_t got;
    while ((got = fread(row.data(), sizeof(uint32_t), row.size(), f)) == row.size())
        printf("%08x\n", words == 3 ? agg_hash<3>(row.data()) : agg_hash<9>(row.data()));
    fclose(f);
    if (got != 0) {
        fprintf(stderr, "%s: %zu words after the last whole tuple\n", argv[2], got);
        return 1;
    }
    return 0;
}
