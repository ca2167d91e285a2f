// Stand-in for the reference's charsets.h: the conversion records its arguments -- the bytes up to
// the size or, without one, up to the first NUL as the reference's strlen does, and the character
// set -- in the byte-keeping QString instead of converting them.
#ifndef FIB_STUB_CHARSETS
#define FIB_STUB_CHARSETS
#include <cstring>
#include "QString"
typedef enum { EbuLatin = 0x00, UnicodeUcs2 = 0x06, UnicodeUtf8 = 0x0F } CharacterSet;
inline QString toQStringUsingCharset(const char *buffer, CharacterSet charset, int size = -1) {
    if (size < 0) size = (int)strlen(buffer);
    QString s;
    s.bytes.assign(buffer, (size_t)size);
    s.pieces.push_back(size);
    s.charsets.push_back((int)charset);
    return s;
}
#endif
