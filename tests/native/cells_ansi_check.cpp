// Stand-alone check of the context-free half of the terminal's cells (all_is_cubes_amd/csrc/aic_cells_host.cpp built with -DAIC_CELLS_HOST_ONLY): random
// grids through aic_cells_ansi at every capacity around the length needed, with guard bytes behind the buffer, and aic_cells_geometry at its edges.
// tests/test_cells_cpu.py builds it with g++ -fsanitize=address,undefined and runs it: its own main, nothing of it is loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/aic_hip.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "cells_ansi_check: %s failed at line %d\n", #cond, __LINE__); return 1; } } while (0)

int main() {
    const char *world[] = {"a", "\xc3\xa9", "\xe6\xbc\xa2", "wide", nullptr, "z"};
    const uint8_t world_w[] = {1, 1, 2, 4, 1, 0};
    const char *ui[] = {"U"};
    const uint32_t glyphs[] = {0x20, '.', 'X', 0x2584, 0x28ff, 0xd800, 0x110000, 0x1f600};
    const uint32_t colours[] = {0, 1u << 24, 2u << 24, (3u << 24) | 231u, (4u << 24) | 0xabcdefu, 9u << 24};
    for (int trial = 0; trial < 300; trial++) {
        const uint32_t cols = rnd() % 9, rows = rnd() % 5;
        std::vector<aic_cell> cells((size_t)cols * rows);
        for (aic_cell &c : cells) {
            c.glyph = (rnd() % 3) ? glyphs[rnd() % 8] : (AIC_CELL_GLYPH_BLOCK | ((rnd() % 3) << 16) | (rnd() % 8));
            c.fg = colours[rnd() % 6];
            c.bg = colours[rnd() % 6];
        }
        aic_cells_text text;
        memset(&text, 0, sizeof(text));
        if (trial % 4) { text.names[0] = world; text.n_names[0] = 6; if (trial % 3) text.widths[0] = world_w; }
        if (trial % 5 == 0) { text.names[1] = ui; text.n_names[1] = 1; }
        text.origin[0] = (uint16_t)(rnd() % 70000u);
        text.origin[1] = (uint16_t)(rnd() % 70000u);
        const uint32_t flags = trial % 2 ? AIC_CELLS_ANSI_IN_RECT : 0u;
        const aic_cells_text *tp = trial % 7 ? &text : nullptr;
        uint64_t need = 0;
        const int rc0 = aic_cells_ansi(cells.data(), cols, rows, tp, flags, nullptr, 0, &need);
        CHECK(need >= 14 && rc0 == AIC_ERR_INVALID);  // hide + reset + reset at the least, and no room for it
        for (uint64_t capacity : {need - 1, need, need + 3}) {
            // exactly `capacity` bytes are the buffer: the sanitizer sees a write past them
            char *buf = (char *)malloc((size_t)capacity);
            memset(buf, 0x5a, (size_t)capacity);
            uint64_t length = 0;
            const int rc = aic_cells_ansi(cells.data(), cols, rows, tp, flags, buf, capacity, &length);
            CHECK(length == need);
            if (capacity < need) {
                CHECK(rc == AIC_ERR_INVALID);
                for (uint64_t i = 0; i < capacity; i++) CHECK(buf[i] == 0x5a);
            } else {
                CHECK(rc == AIC_OK && memcmp(buf, "\x1b[?25l\x1b[0m", 10) == 0 && memcmp(buf + need - 4, "\x1b[0m", 4) == 0);
                for (uint64_t i = need; i < capacity; i++) CHECK(buf[i] == 0x5a);
            }
            free(buf);
        }
    }
    uint32_t w = 0, h = 0;
    double nominal[2];
    CHECK(aic_cells_geometry(0, 0, AIC_CELLS_BRAILLE, &w, &h, nominal) == AIC_OK && w == 2 && h == 4 && nominal[0] == 0.5 && nominal[1] == 1.0);
    CHECK(aic_cells_geometry(65535, 65535, AIC_CELLS_BRAILLE, &w, &h, nullptr) == AIC_OK && w == 131070u && h == 262140u);
    CHECK(aic_cells_geometry(65536, 1, AIC_CELLS_SPLIT, &w, &h, nullptr) == AIC_ERR_INVALID && aic_cells_geometry(1, 1, 5, nullptr, nullptr, nullptr) == AIC_ERR_INVALID);
    printf("cells_ansi_check ok\n");
    return 0;
}
