// The 5 x 7 font of the preview sheet's TEXT panels (sheet.hip): thirteen glyphs, the characters "0123456789.-" and
// the space, in that order.  A glyph is seven rows from the top; bit 4 of a row is its leftmost column.  Host and device both read it: the entry
// point translates a panel's characters into glyph indices (sheet_glyph_index), the kernel looks the rows up.
#pragma once
#include <stdint.h>

#define CS_SHEET_GLYPHS 13
#define CS_SHEET_CHARS "0123456789.- "
// clang-format off
#define CS_SHEET_FONT_ROWS                                                   \
  {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, /* 0 */                        \
  {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, /* 1 */                        \
  {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F}, /* 2 */                        \
  {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, /* 3 */                        \
  {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, /* 4 */                        \
  {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E}, /* 5 */                        \
  {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, /* 6 */                        \
  {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, /* 7 */                        \
  {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E}, /* 8 */                        \
  {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, /* 9 */                        \
  {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C}, /* . */                        \
  {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00}, /* - */                        \
  {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00}  /* space */
// clang-format on

// index of a character in CS_SHEET_CHARS, -1 for any other
static inline int sheet_glyph_index(char c) {
  const char* set = CS_SHEET_CHARS;
  for (int i = 0; i < CS_SHEET_GLYPHS; ++i)
    if (set[i] == c) return i;
  return -1;
}
