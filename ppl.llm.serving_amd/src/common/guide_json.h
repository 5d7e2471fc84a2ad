// Guided decoding by a JSON schema (DESIGN.md "numerics", guided decoding row): the schema becomes a wide byte-level automaton
// (GuideDfa16, guide.h) whose language is the UTF-8 JSON text of the documents that fit it, in ONE fixed layout.  The schema is read
// with utils::JsonValue (its `keys` keep the document order of `properties`); the syntax tree is built directly and goes through the
// same NFA -> subset construction -> trim -> minimisation as a regular expression (guide_tree.h).
//
// Layout: one optional space in front of the value (the first piece of a SentencePiece answer carries one), one optional space behind
// every ':' and every ','; no whitespace anywhere else.
// Strings: the escapes \" \\ \/ \b \f \n \r \t \uXXXX; no raw byte below 0x20; besides ASCII only well-formed UTF-8 of 2 .. 4 bytes (no
// surrogates, no overlong forms, nothing above U+10FFFF).  minLength / maxLength count characters, an escape being one (an escaped
// surrogate pair too; a lone escaped surrogate is not produced); bounds <= 256.
// Numbers: integer = -?(0|[1-9][0-9]{0,17}); number adds (\.[0-9]{1,17})?([eE][+-]?[0-9]{1,3})?.
// Keywords: type (a name or a list of names among object string integer number boolean null array); properties (emitted in the schema's
// order), required (a property outside it may be left out; the commas stay right), additionalProperties (read and ignored: nothing
// undeclared is ever produced); items, minItems, maxItems (<= 256); enum / const of scalars (serialised canonically; beside `type` the
// values of that type); anyOf; $ref to #/$defs/NAME or #/definitions/NAME; the annotations title description default examples $schema
// $id format are skipped.
// Refused, with the keyword and its JSON pointer in the message: a recursive $ref; a schema or `items` without a type (any value would be
// recursive); every other keyword (oneOf allOf not if then else pattern patternProperties minimum maximum multipleOf uniqueItems
// prefixItems ...); an enum of non-scalars; a bound above 256; enum, const, anyOf or $ref beside other constraints; a schema that matches
// nothing; an enum number that is not finite; a schema whose nesting expands to more than 200,000 syntax nodes (an array keeps its
// item twice, an object a member once per member that may come first, a $ref is expanded at every use: the tree can double per level,
// so the compiler bounds its own work); an automaton of more than 65,534 states before minimisation or more than 4096 after it (both
// numbers in the message).
#pragma once
#include <string>

#include "guide.h"

namespace ppl { namespace llm {

constexpr size_t kGuideJsonMaxSubsetStates = 65534;

// false: *err says why; *dfa is unspecified
bool CompileGuideJsonSchema(const std::string& schema, GuideDfa16* dfa, std::string* err);

}}  // namespace ppl::llm
