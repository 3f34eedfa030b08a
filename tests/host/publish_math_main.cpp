// publish_math_main.cpp -- csrc/publish_math.h on the host: reads requests (one per line) from argv[1], writes the answers to argv[2].
//   I <16 hex words: T>   ->   I <16 hex words: the inverse>   or   I singular
#include "publish_math.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "r"); FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    char op;
    while (fscanf(in, " %c", &op) == 1) {
        if (op != 'I') return 3;
        float T[16], Ti[16];
        for (int k = 0; k < 16; k++) { unsigned w; if (fscanf(in, "%x", &w) != 1) return 3; uint32_t u = w; memcpy(&T[k], &u, 4); }
        if (!pub_inverse4(T, Ti)) { fprintf(out, "I singular\n"); continue; }
        fprintf(out, "I");
        for (int k = 0; k < 16; k++) { uint32_t u; memcpy(&u, &Ti[k], 4); fprintf(out, " %08x", u); }
        fprintf(out, "\n");
    }
    fclose(in); fclose(out);
    return 0;
}
