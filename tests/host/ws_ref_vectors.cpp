// ws_ref_vectors.cpp -- drives the reference's own ws_decoder_t and
// ws_encoder_t for tests/golden/make_ws_vectors.py, which compiles this file
// together with the reference's src/msg.cpp, metadata.cpp, err.cpp,
// ws_decoder.cpp, decoder_allocators.cpp and ws_encoder.cpp where they lie
// (tests/host/ref_platform/platform.hpp in place of the generated one) and
// records what it prints in tests/golden/ws_vectors.json.
//
// One command per line on stdin, one answer line on stdout:
//   D <must_mask> <maxmsgsize> <step> <hex>
//       the bytes fed to a fresh decoder the way the engine's in_event does
//       (get_buffer, copy, decode until the chunk is used), all at once
//       (step 0) or one byte per read (step 1):
//       "<rc> <fed> <errno> <n> {<flags> <hex>}*n" -- rc -1 after a failure
//       (fed: the stream bytes the decoder had taken when it failed, errno as
//       the decoder left it, 0 where it sets none), 0 otherwise; then the
//       messages in order with their msg_t flags and their (unmasked) bytes
//   E <must_mask> <random> <flags> <hex>
//       one message with these msg_t flags through a fresh encoder whose
//       generate_random() returns <random>: "<hex of the frame>"
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "precompiled.hpp"
#include "zmq.h"
#include "msg.hpp"
#include "ws_decoder.hpp"
#include "ws_encoder.hpp"

static uint32_t g_random;

// (src/random.cpp is not linked: the mask key is the test's)
namespace zmq
{
uint32_t generate_random ()
{
    return g_random;
}
}

static std::vector<unsigned char> unhex (const std::string &s)
{
    std::vector<unsigned char> v;
    if (s == "-")
        return v;
    for (size_t i = 0; i + 1 < s.size (); i += 2)
        v.push_back ((unsigned char) strtoul (s.substr (i, 2).c_str (), NULL, 16));
    return v;
}

static std::string hex (const unsigned char *p, size_t n)
{
    static const char d[] = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return n ? s : "-";
}

static void decode_case (bool must_mask, int64_t maxmsg, int step, const std::vector<unsigned char> &in)
{
    zmq::ws_decoder_t dec (8192, maxmsg, true, must_mask);
    std::ostringstream msgs;
    size_t pos = 0, count = 0, fed = 0;
    int rc = 0, err = 0;
    while (pos < in.size () && rc != -1) {
        unsigned char *buf;
        size_t room;
        dec.get_buffer (&buf, &room);
        const size_t chunk = std::min (room, step ? (size_t) 1 : in.size () - pos);
        memcpy (buf, &in[pos], chunk);
        dec.resize_buffer (chunk);
        size_t off = 0;
        while (off < chunk) {
            size_t used = 0;
            errno = 0;
            rc = dec.decode (buf + off, chunk - off, used);
            off += used;
            if (rc == -1) {
                err = errno;
                fed = pos + off;
                break;
            }
            if (rc == 1) {
                zmq::msg_t *m = dec.msg ();
                msgs << ' ' << (unsigned) (m->flags () & ~zmq::msg_t::shared) << ' '
                     << hex ((const unsigned char *) m->data (), m->size ());
                ++count;
            }
        }
        pos += chunk;
    }
    std::cout << rc << ' ' << (rc == -1 ? fed : pos) << ' ' << err << ' ' << count << msgs.str () << std::endl;
}

static void encode_case (bool must_mask, uint32_t random, unsigned flags, const std::vector<unsigned char> &body)
{
    g_random = random;
    zmq::ws_encoder_t enc (8192, must_mask);
    zmq::msg_t m;
    int rc = m.init_size (body.size ());
    if (rc != 0)
        abort ();
    if (!body.empty ())
        memcpy (m.data (), &body[0], body.size ());
    m.set_flags ((unsigned char) flags);
    enc.load_msg (&m);
    std::vector<unsigned char> out;
    for (;;) {
        unsigned char *p = NULL;
        const size_t k = enc.encode (&p, 0);
        if (k == 0)
            break;
        out.insert (out.end (), p, p + k);
    }
    std::cout << hex (out.empty () ? NULL : &out[0], out.size ()) << std::endl;
}

int main ()
{
    std::string line;
    while (std::getline (std::cin, line)) {
        std::istringstream ss (line);
        std::string cmd, data;
        ss >> cmd;
        if (cmd == "D") {
            int must_mask, step;
            long long maxmsg;
            ss >> must_mask >> maxmsg >> step >> data;
            decode_case (must_mask != 0, maxmsg, step, unhex (data));
        } else if (cmd == "E") {
            int must_mask;
            unsigned long random;
            unsigned flags;
            ss >> must_mask >> random >> flags >> data;
            encode_case (must_mask != 0, (uint32_t) random, flags, unhex (data));
        }
    }
    return 0;
}
