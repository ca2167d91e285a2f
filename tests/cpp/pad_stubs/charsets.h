// Stand-in for the reference's charsets.h: the conversion records its arguments -- the bytes,
// the character set and the size -- in the byte-keeping QString instead of converting them.
#ifndef PAD_STUB_CHARSETS
#define PAD_STUB_CHARSETS
#include <cstdio>
#include <cstdlib>
#include "QString"
typedef enum { EbuLatin = 0x00, UnicodeUcs2 = 0x06, UnicodeUtf8 = 0x0F } CharacterSet;
inline QString toQStringUsingCharset(const char *buffer, CharacterSet charset, int size = -1) {
    if (size < 0) {
        fprintf(stderr, "toQStringUsingCharset: size %d\n", size);
        abort();
    }
    QString s;
    s.bytes.assign(buffer, (size_t)size);
    s.pieces.push_back(size);
    s.charsets.push_back((int)charset);
    return s;
}
#endif
